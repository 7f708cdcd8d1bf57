"""Parameter gradients of the decoder / head linears and LayerNorms: which kernel computes a dW / db, and when.

Inside `deferred_param_grads()` a parameter used ONCE in the forward hands autograd a freshly allocated, UNWRITTEN placeholder and
queues its operands; the flush at the end of the scope writes all of them - into whatever tensor autograd stored as `.grad` - with
one batched launch per shape (u3d_wgrad_batched_bf16 / u3d_colsum_batched): ~45 independent [N x 7200] x [7200 x K] products of
14 us each become two launches.  Valid because nothing reads a parameter gradient before the flush: with `.grad = None`
AccumulateGrad keeps the incoming tensor as is (a weight used twice would accumulate, hence the census USES; no reference to the
placeholder is kept here, so it is not cloned either).  The route says once, from plain values, where a dW and a db come from.
"""
import contextlib
import functools
from typing import NamedTuple

import torch

from .. import native as nv


class ParamUses:
    """Census of one step's forward: how often each weight was used, and how many of those uses were fused decoder layers."""

    def __init__(self):
        self.count, self.fused, self.params = {}, {}, {}          # id(weight) -> uses / fused uses / (weight, bias)

    def note(self, weight, bias, fused=False):
        wid = id(weight)
        self.count[wid], self.fused[wid], self.params[wid] = self.count.get(wid, 0) + 1, self.fused.get(wid, 0) + bool(fused), (weight, bias)
        return wid

    def single(self, weight):
        return self.count.get(id(weight), 0) == 1

    def all_fused(self, weight):
        return self.fused.get(id(weight), 0) == self.count.get(id(weight), 0)


USES = ParamUses()


def reset_param_uses():
    USES.__init__()


class GradQueue:
    """What one deferred_param_grads() scope has queued, in backward execution order.  The flush sorts each launch group by output
    pointer, STABLY: items with one output (a linear shared by several layers) get consecutive batch slots and the kernel sums them."""

    def __init__(self):
        self.products = []        # (dy [M,N], x [M,K], weight, bias or None, first row, last row): wide dW (+ db) of weight[r0:r1]
        self.skinny = []          # (dy [M,n], x [M,k], weight) with min(n, k) <= 16: all products of a step in one launch per M
        self.sums = []            # (matrix [rows, C], parameter): parameter.grad <- column sums
        self.shared_seen = set()  # weights with several uses whose placeholder has been handed to autograd in this backward

    def product(self, dy, x, weight, bias, r0, r1):
        self.products.append((dy, x, weight, bias, r0, r1))

    def skinny_product(self, dy, x, weight):
        self.skinny.append((dy, x, weight))

    def colsum(self, mat, param):
        self.sums.append((mat, param))

    def first_use(self, weight):      # the first backward of a shared weight hands autograd the placeholder, the others None
        first = id(weight) not in self.shared_seen
        self.shared_seen.add(id(weight))
        return first

    def flush(self):
        """Returns the operands the launches read: a caller that flushes on a side stream keeps them alive until the streams join."""
        keep = products, sums, skinny = self.products, self.sums, self.skinny
        self.__init__()
        by_m = {}
        for it in skinny:
            by_m.setdefault(it[0].shape[0], []).append(it)
        for lst in by_m.values():
            parts = nv.skinny_wgrad_partial_batched([d for d, _, _ in lst], [x for _, x, _ in lst])
            sums = sums + [(p, w) for p, (_, _, w) in zip(parts, lst)]
        groups, bgroups = {}, {}
        for mat, param in sums:                   # LayerNorm dgamma / dbeta, skinny dW / db, narrow linears' db
            g = param.grad
            if g is None or g.dtype != torch.float32 or not g.is_contiguous() or g.numel() != mat.shape[1]:
                raise RuntimeError("deferred column sum: no matching contiguous f32 .grad to write into")
            bgroups.setdefault((mat.shape[0], mat.shape[1], str(mat.dtype)), []).append((mat, g))
        for dy, x, w, b, r0, r1 in products:
            if w.grad is None or w.grad.dtype != torch.float32 or not w.grad.is_contiguous():
                raise RuntimeError("deferred weight gradient: autograd did not leave a contiguous f32 .grad to write into")
            groups.setdefault((dy.shape[0], dy.shape[1], x.shape[1]), []).append((dy, x, w.grad[r0:r1]))
            if b is not None:
                if b.grad is None or b.grad.dtype != torch.float32:
                    raise RuntimeError("deferred bias gradient: no f32 .grad to write into")
                bgroups.setdefault((dy.shape[0], dy.shape[1]), []).append((dy, b.grad[r0:r1]))
        for g in groups.values():
            g.sort(key=lambda t: t[2].data_ptr())
            nv.wgrad_batched([a for a, _, _ in g], [b for _, b, _ in g], [c for _, _, c in g])
        for g in bgroups.values():
            g.sort(key=lambda t: t[1].data_ptr())
            nv.colsum_batched([a for a, _ in g], [b for _, b in g])
        return keep


QUEUE = None      # the innermost open scope's queue; None outside deferred_param_grads()


def flush_deferred():
    return QUEUE.flush() if QUEUE is not None else ([], [], [])


@contextlib.contextmanager
def deferred_param_grads():
    global QUEUE
    prev, QUEUE = QUEUE, GradQueue()
    try:
        yield
        QUEUE.flush()
    finally:
        QUEUE = prev              # an exception drops what was queued


# Where a gradient comes from.  Written by the flush (autograd gets a placeholder): queue (wide product in the batched bf16 launch;
# as db: the bias sum that rides with it), queue_shared (the same for a linear used by several fused layers: ONE placeholder, the
# launch sums the uses), skinny_queue (batched skinny launch), partial_queue (skinny partials now, their sum queued), sum_queue (column
# sum queued).  In this backward: batch / split (the fused layer's own batched bf16 launch; split: f32 operands as three products of
# bf16 hi / lo planes), partial (skinny partials + their sum), own (u3d_spconv_wgrad, one offset), blas (torch matmul), sum.
DW = ("queue", "queue_shared", "skinny_queue", "partial_queue", "sum_queue", "batch", "split", "partial", "own", "blas", "sum", None)
DB = ("queue", "sum_queue", "sum", None)


class Route(NamedTuple):
    dw: str               # one of DW (a LayerNorm's gamma counts as dW, its beta as db)
    db: str               # one of DB
    grad_view: bool       # the placeholder may be the parameter's `_u3d_grad_view` (nothing but the flush writes it)


@functools.lru_cache(maxsize=4096)          # plain hashable values in, an immutable record out: nothing allocated per call
def layer_route(kind, active, single, need_dw, need_db, bf16=False, m=0, n=0, k=0, has_bias=True, on_gpu=True, own_wgrad=True,
                skinny_wgrad=False):
    """Layer-by-layer path.  kind: "linear" (y = x W^T + b, [m,k] -> [m,n]), "inproj" (one half of the packed in-projection: the
    pair (dW, db) is produced whenever dW is wanted, need_db = the bias wants one too) or "norm" (LayerNorm: no shape or toggle
    matters).  own_wgrad / skinny_wgrad: transformer.OWN_WGRAD / SKINNY_WGRAD at the time of the call."""
    if kind == "norm":
        s = "sum_queue" if (active and single and need_dw and need_db) else "sum"
        return Route(s, s, False)
    if kind == "inproj":
        ok, need_db = active and single and need_dw and need_db, need_dw
    else:
        ok = active and single and (need_db or not has_bias)
    own = bf16 and own_wgrad and m > 0
    if ok and need_dw and own and n % 64 == 0 and k % 64 == 0:
        return Route("queue", "queue" if need_db else None, False)
    if need_dw and own and skinny_wgrad and min(n, k) <= 16 and kind == "linear":
        return Route("partial_queue" if ok else "partial", ("sum_queue" if ok else "sum") if need_db else None, False)
    dw = None if not need_dw else "own" if (own and n % 16 == 0 and k % 16 == 0) else "blas"
    # narrow linears (N or K no multiple of 64) keep their own dW path, but the bias sum joins the batched sums
    db = None if not need_db else "sum_queue" if (ok and kind == "linear" and on_gpu) else "sum"
    return Route(dw, db, False)


@functools.lru_cache(maxsize=4096)
def fused_route(kind, active, bf16, n, k, single, all_fused, split_f32_wgrad, shared_defer):
    """Fused decoder layer.  kind: "wide", "inproj" (packed half), "narrow" (reg / cls / iou final layer), "skinny" (attention_weights,
    position encoder input) or "norm".  The queued launches are bf16 kernels: f32 layers compute every product in their backward."""
    defer = active and bf16
    if kind == "norm":
        return Route("sum_queue", "sum_queue", True) if (defer and single) else Route("sum", "sum", False)
    if kind in ("narrow", "skinny"):
        return Route("skinny_queue", "sum_queue", True) if (defer and single) else Route("partial" if bf16 else "own", "sum", False)
    if shared_defer and defer and not single and kind == "wide" and all_fused:
        return Route("queue_shared", "queue", True)
    if defer and single:
        return Route("queue", "queue", True)
    return Route("batch" if bf16 else "split" if (split_f32_wgrad and n % 64 == 0 and k % 64 == 0) else "own", "sum", False)
