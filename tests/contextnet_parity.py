"""Helpers of the ContextNet parity tests (tests/test_contextnet_parity_gpu.py, tests/test_contextnet_store_hook.py): the oracle of ONE
block with autograd, the straight-through bf16 rounding passed to the oracle's `store=` hook, relative-L2 distances per parameter
family, and recorders of which weight-gradient route a module took on the GPU path."""
import torch

from oracle import contextnet_ref as R

FAMILIES = ("dw", "pw", "bn", "se")


def l_config():
    from tensorflowasr_amd import configs

    return configs.contextnet(alpha=2.0)          # ContextNet-L: 23 blocks, widths 512 / 1024 / 1280, time reduction 8


def round_bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def store_bf16(x):
    """Straight-through bf16 storage: the forward value is rounded (x + (round(x) - x) is exactly round(x): the difference is exact and
    the sum is representable), the gradient that arrives at the stored tensor is rounded by a hook."""
    y = x + (round_bf16(x.detach()) - x.detach())
    if y.requires_grad:
        y.register_hook(round_bf16)
    return y


def rel_l2(a, b):
    """||a - b|| / ||b|| in f64."""
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / b.norm().clamp(min=1e-300))


def block_param_names(blk):
    names = []
    for (m, *_rest) in blk["convs"] + ([blk["res"]] if blk["res"] else []):
        names += [m + "/dw", m + "/pw/w", m + "/pw/b", m + "/bn/g", m + "/bn/b"]
    p = blk["prefix"] + "se/"
    return names + [p + "fc1/w", p + "fc1/b", p + "fc2/w", p + "fc2/b"]


def family(name):
    if "/se/fc" in name:
        return "se"
    for f, tail in (("dw", "/dw"), ("pw", "/pw/w"), ("pw", "/pw/b"), ("bn", "/bn/g"), ("bn", "/bn/b")):
        if name.endswith(tail):
            return f
    raise KeyError(name)


def by_family(grads):
    """name -> tensor  =>  family -> one flat f64 vector (names in sorted order)."""
    out = {}
    for f in FAMILIES:
        parts = [grads[k].double().reshape(-1) for k in sorted(grads) if family(k) == f]
        out[f] = torch.cat(parts)
    return out


def module_key(blk, mod):
    """(Cin, Cout, K, stride, has_residual): the distinct conv-module shapes of a configuration."""
    _m, ci, co, Kk, s, _act = mod
    return (ci, co, Kk, s, blk["res"] is not None)


def module_keys(blocks):
    return {module_key(blk, m) for blk in blocks for m in blk["convs"] + ([blk["res"]] if blk["res"] else [])}


def oracle_block(x, lens, W, blk, dy, dtype, store=None):
    """Autograd through one block: leaves are the block's input and its weights.  Returns y, dx, {name: grad}, lengths (all `dtype`)."""
    Wb = {k: W[k].to(dtype).clone().requires_grad_(True) for k in block_param_names(blk)}
    xi = x.to(dtype).clone().requires_grad_(True)
    kw = {} if store is None else dict(store=store)
    y, lens2 = R.encoder_forward(xi, lens, Wb, [blk], **kw)
    y.backward(dy.to(dtype))
    return y.detach(), xi.grad, {k: v.grad for k, v in Wb.items()}, lens2


def distances(got, ref):
    """(y, dx, grads) triples -> {"y", "dx", "dw", "pw", "bn", "se"} relative-L2 distances of `got` from `ref`."""
    d = {"y": rel_l2(got[0], ref[0]), "dx": rel_l2(got[1], ref[1])}
    fg, fr = by_family(got[2]), by_family(ref[2])
    for f in FAMILIES:
        d[f] = rel_l2(fg[f], fr[f])
    return d


class Routes:
    """Which route each pointwise weight gradient took, and what the grouped / batched launches looked like."""

    def __init__(self):
        self.base, self.queued = [], []          # weight names: AsrModel._dense_bwd / the queue of ContextNetTransducer
        self.groups = []                         # (products, kernel launches) per K.gemm_group call
        self.many = []                           # (items, x shape, K) per K.dwconv_bwd_weight_many call
        self.dw_single = 0                       # K.dwconv_bwd_weight calls

    def clear(self):
        self.__init__()


def instrument(monkeypatch):
    """Count K.gemm_group / K.dwconv_bwd_weight_many / K.dwconv_bwd_weight calls and record the route of every _dense_bwd."""
    from tensorflowasr_amd import kernels as K
    from tensorflowasr_amd.contextnet import ContextNetTransducer
    from tensorflowasr_amd.model import AsrModel

    rec = Routes()
    group0, many0, single0 = K.gemm_group, K.dwconv_bwd_weight_many, K.dwconv_bwd_weight
    base0, cn0 = AsrModel._dense_bwd, ContextNetTransducer._dense_bwd

    def group(calls):
        n0 = K.launch_count()
        group0(calls)
        rec.groups.append((len(calls), K.launch_count() - n0))

    def many(items):
        rec.many.append((len(items), tuple(items[0][0].shape), int(items[0][2].shape[0])))
        return many0(items)

    def single(*a, **k):
        rec.dw_single += 1
        return single0(*a, **k)

    def base(self, dy, x, wname, *a, **k):
        rec.base.append(wname)
        return base0(self, dy, x, wname, *a, **k)

    def cn(self, dy, x, wname, *a, **k):
        n0 = len(rec.base)
        out = cn0(self, dy, x, wname, *a, **k)
        if len(rec.base) == n0:
            rec.queued.append(wname)
        return out

    monkeypatch.setattr(K, "gemm_group", group)
    monkeypatch.setattr(K, "dwconv_bwd_weight_many", many)
    monkeypatch.setattr(K, "dwconv_bwd_weight", single)
    monkeypatch.setattr(AsrModel, "_dense_bwd", base)
    monkeypatch.setattr(ContextNetTransducer, "_dense_bwd", cn)
    return rec


def shadow_per_layer(monkeypatch, model):
    """During ONE backward pass, launch the per-layer weight gradient of every conv module (the base route's split-K GEMM with the bias
    column sums, K.dwconv_bwd_weight) into a second flat gradient buffer, on the SAME operands, at the moment the model queues them.
    The queued routes read those operands later (at the flush): an operand overwritten in between, a lost or doubled queue entry or a
    wrong slice shows as a difference, and nothing else does.  Call before instrument().  Returns the second buffer."""
    from tensorflowasr_amd import kernels as K
    from tensorflowasr_amd.conformer import _split_k
    from tensorflowasr_amd.contextnet import ContextNetTransducer

    alt = torch.zeros_like(model.ps.grad)
    assert model.ps.grad.storage_offset() == 0 and model.ps.grad.dim() == 1
    gemm0, single0 = K.gemm, K.dwconv_bwd_weight
    cn0, cm0 = ContextNetTransducer._dense_bwd, ContextNetTransducer._cm_bwd

    def view(t):
        return alt.as_strided(tuple(t.shape), tuple(t.stride()), t.storage_offset())

    def cn(self, dy, x, wname, bname, *a, **k):
        if wname.endswith("/pw/w"):
            din, dout = self.ps.w2d(wname).shape
            rows = dy.shape[0]
            gemm0(x, dy, view(self.ps.g2d(wname)), din, dout, rows, x.stride(0), dy.stride(0), dout, trans_a=True, accumulate=True,
                  split_k=_split_k(din, dout, rows), colsum=view(self.ps.g(bname)))
        return cn0(self, dy, x, wname, bname, *a, **k)

    def cm(self, dy, mod, B, ctx):
        q = self._dw_queue
        n0 = len(q)
        out = cm0(self, dy, mod, B, ctx)
        assert len(q) == n0 + 1
        single0(q[-1][0], q[-1][1], view(q[-1][2]), None)
        return out

    monkeypatch.setattr(ContextNetTransducer, "_dense_bwd", cn)
    monkeypatch.setattr(ContextNetTransducer, "_cm_bwd", cm)
    return alt
