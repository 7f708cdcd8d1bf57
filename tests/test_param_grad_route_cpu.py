"""plugin/param_grads.py without a GPU: the route (where a decoder / head parameter's dW and db come from, decided once) against the
expressions _linear_backward, _TorchLinearFn, _InProjFn, _FusedLN and FusedLayerFn.backward carried piecemeal before it, and the
bookkeeping of the queue one deferred_param_grads() scope owns, with the three batched launches replaced by recorders."""
import itertools

import pytest
import torch

from uni3detr_amd import native as nv
from uni3detr_amd.plugin import param_grads as PG

NK = ((256, 256), (512, 256), (256, 384), (10, 256), (1, 256), (256, 3), (48, 48))
BOOLS = (True, False)


def layer_route_as_it_was(kind, active, uses, bf16, m, n, k, need_dw, need_db, has_bias, on_gpu, OWN_WGRAD, SKINNY_WGRAD):
    """_TorchLinearFn / _InProjFn / _FusedLN .backward followed by _linear_backward, branch by branch.  need_dw / need_db are
    ctx.needs_input_grad of the weight / the bias."""
    if kind == "norm":                                           # _FusedLN.backward
        if active and uses == 1 and need_dw and need_db:
            return "sum_queue", "sum_queue", False
        return "sum", "sum", False
    if kind == "linear":                                         # _TorchLinearFn.backward
        need_db = has_bias and need_db
        ok = active and uses == 1 and (need_db or not has_bias)
        defer = (0, n) if ok else None
        outs = False
    else:                                                        # _InProjFn.backward: need_w for both, slices of one (dw, db) pair
        need_w = need_dw
        ok = active and uses == 1 and need_w and need_db
        defer = ((0, n) if n == 512 else (512, 512 + n)) if ok else None
        need_dw = need_db = need_w
        outs = bool(need_w)
    # _linear_backward
    if defer is not None and need_dw and bf16 and OWN_WGRAD and n % 64 == 0 and k % 64 == 0 and m > 0:
        return "queue", ("queue" if need_db else None), False
    if need_dw and bf16 and OWN_WGRAD and SKINNY_WGRAD and m > 0 and min(n, k) <= 16 and not outs:
        if defer is not None and defer[0] == 0 and defer[1] == n:
            return "partial_queue", ("sum_queue" if need_db else None), False
        return "partial", ("sum" if need_db else None), False
    dw = db = None
    if need_dw:
        if bf16 and OWN_WGRAD and n % 16 == 0 and k % 16 == 0 and m > 0:
            dw = "own"
        else:
            dw = "blas"                                          # _mm_f32 for bf16 operands, a plain product else
    if need_db:
        if defer is not None and active and not outs and defer[0] == 0 and defer[1] == n and on_gpu and has_bias:
            db = "sum_queue"
        else:
            db = "sum"
    return dw, db, False


def fused_route_as_it_was(kind, active, uses, fused_uses, bf16, n, k, split_f32_wgrad, SHARED_DEFER):
    """FusedLayerFn.backward: the linear loop, the LayerNorm loop and the attention_weights / pe0 loop."""
    deferred_ok = active and bf16
    single = uses == 1
    dfr = deferred_ok and uses == 1                              # what slot() was called with
    if kind == "norm":
        return ("sum_queue", "sum_queue", dfr) if (deferred_ok and uses == 1) else ("sum", "sum", dfr)
    if kind == "skinny":
        if deferred_ok and uses == 1:
            return "skinny_queue", "sum_queue", dfr
        return ("partial" if bf16 else "own"), "sum", dfr       # skinny_now
    shared = SHARED_DEFER and deferred_ok and not single and kind != "narrow" and kind != "inproj" and fused_uses == uses
    if shared:
        return "queue_shared", "queue", True                     # slot(w, True) for the first, None for the others
    if kind == "narrow":
        if deferred_ok and single:
            return "skinny_queue", "sum_queue", dfr
        return ("partial" if bf16 else "own"), "sum", dfr
    if deferred_ok and single:
        return "queue", "queue", dfr
    if bf16:
        return "batch", "sum", dfr
    if split_f32_wgrad and n % 64 == 0 and k % 64 == 0:
        return "split", "sum", dfr
    return "own", "sum", dfr


def test_route_is_what_the_five_backward_bodies_decided_piecemeal():
    seen = set()
    census = [(u, f) for u in (1, 2, 3) for f in range(u + 1)]
    for active, bf16, (uses, fused), (n, k), m, need_dw, need_db, has_bias, on_gpu, own, skinny in itertools.product(
            BOOLS, BOOLS, census, NK, (0, 40), BOOLS, BOOLS, BOOLS, BOOLS, BOOLS, BOOLS):
        for kind in ("linear", "inproj", "norm"):
            if kind == "inproj" and (not has_bias or (n, k) not in ((512, 256), (256, 256))):
                continue                                         # the packed in-projection: [512 + 256, 256] with a bias
            want = layer_route_as_it_was(kind, active, uses, bf16, m, n, k, need_dw, need_db, has_bias, on_gpu, own, skinny)
            # _TorchLinearFn asked for db only when there is a bias
            r = PG.layer_route(kind, active, uses == 1, need_dw, (has_bias and need_db) if kind == "linear" else need_db, bf16, m, n, k,
                               has_bias=has_bias, on_gpu=on_gpu, own_wgrad=own, skinny_wgrad=skinny)
            assert tuple(r) == want, (kind, active, bf16, uses, n, k, m, need_dw, need_db, has_bias, on_gpu, own, skinny)
            seen.add(r)
    for active, bf16, split, (uses, fused), (n, k), shared_defer in itertools.product(BOOLS, BOOLS, BOOLS, census, NK, BOOLS):
        for kind in ("wide", "inproj", "narrow", "skinny", "norm"):
            want = fused_route_as_it_was(kind, active, uses, fused, bf16, n, k, split, shared_defer)
            r = PG.fused_route(kind, active, bf16, n, k, uses == 1, fused == uses, split, shared_defer)
            assert tuple(r) == want, (kind, active, bf16, split, uses, fused, n, k, shared_defer)
            seen.add(r)
    # every source the record can name is reached, and grad-view placement only by what the flush alone writes
    assert {r.dw for r in seen} == set(PG.DW) and {r.db for r in seen} == set(PG.DB)
    assert {(r.dw, r.db) for r in seen if r.grad_view} == {("queue", "queue"), ("queue_shared", "queue"), ("skinny_queue", "sum_queue"),
                                                            ("sum_queue", "sum_queue")}
    with pytest.raises(AttributeError):
        r.dw = None             # the record is immutable: a caller cannot "re-decide" into it


def test_layer_path_never_places_a_gradient_view():
    for kind, active, single, dw, db in itertools.product(("linear", "inproj", "norm"), BOOLS, BOOLS, BOOLS, BOOLS):
        assert not PG.layer_route(kind, active, single, dw, db, True, 40, 256, 256).grad_view


def test_census_counts_uses_and_fused_uses():
    w, b, v = torch.zeros(2, 2), torch.zeros(2), torch.zeros(3)
    PG.reset_param_uses()
    assert not PG.USES.single(w) and id(w) not in PG.USES.params
    wid = PG.USES.note(w, b, fused=True)
    assert wid == id(w) and PG.USES.single(w) and PG.USES.all_fused(w) and PG.USES.params[wid][0] is w and PG.USES.params[wid][1] is b
    PG.USES.note(w, b)
    PG.USES.note(v, None)
    assert not PG.USES.single(w) and not PG.USES.all_fused(w) and PG.USES.single(v) and not PG.USES.fused.get(id(v))
    uses = PG.USES
    PG.reset_param_uses()
    assert PG.USES is uses and not PG.USES.single(v) and PG.USES.count == {}     # the object stays, its contents go


# ---- the queue: the three batched launches recorded instead of run ---------------------------------------------------------------------

class FakeTensor:
    """What the flush looks at: shape, dtype, data_ptr, slicing of a gradient, .grad."""

    def __init__(self, shape, ptr=0, dtype=torch.bfloat16, grad=None, name=None):
        self.shape, self.ptr, self.dtype, self.grad, self.name = tuple(shape), ptr, dtype, grad, name

    def data_ptr(self):
        return self.ptr

    def is_contiguous(self):
        return True

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def __getitem__(self, sl):
        row = self.numel() // self.shape[0]
        return FakeTensor((sl.stop - sl.start,) + self.shape[1:], self.ptr + 4 * row * sl.start, self.dtype, name=(self.name, sl.start, sl.stop))


def param(shape, ptr, name):
    return FakeTensor(shape, grad=FakeTensor(shape, ptr, torch.float32, name=name))


@pytest.fixture
def launches(monkeypatch):
    log = []
    monkeypatch.setattr(nv, "wgrad_batched", lambda ins, douts, dws: log.append(("wgrad", list(ins), list(douts), list(dws))))
    monkeypatch.setattr(nv, "colsum_batched", lambda xs, outs: log.append(("colsum", list(xs), list(outs))))

    def partials(dys, xs):
        log.append(("skinny", list(dys), list(xs)))
        return [FakeTensor((57, d.shape[1] * x.shape[1]), dtype=torch.float32, name=("partial", d.name)) for d, x in zip(dys, xs)]
    monkeypatch.setattr(nv, "skinny_wgrad_partial_batched", partials)
    return log


def test_flush_groups_by_shape_and_sorts_stably_by_output_pointer(launches):
    M = 40
    dy = lambda n, name: FakeTensor((M, n), name=name)          # noqa: E731
    w_hi, b_hi = param((256, 256), 9000000, "w_hi"), param((256,), 900000, "b_hi")
    w_lo, b_lo = param((256, 256), 1000, "w_lo"), param((256,), 100, "b_lo")            # lower address, queued later
    w_in, b_in = param((768, 256), 5000, "w_in"), param((768,), 500, "b_in")
    w_nb = param((256, 384), 7000, "w_nb")
    w_sk, b_sk, gam = param((10, 256), 3000, "w_sk"), param((10,), 300, "b_sk"), param((256,), 200, "gamma")
    with PG.deferred_param_grads():
        q = PG.QUEUE
        d = [dy(256, "d%d" % i) for i in range(4)]
        x = [FakeTensor((M, 256), name="x%d" % i) for i in range(4)]
        q.product(d[0], x[0], w_hi, b_hi, 0, 256)                # a shared weight: three uses, interleaved with another weight's
        q.product(d[1], x[1], w_lo, b_lo, 0, 256)
        q.product(d[2], x[2], w_hi, b_hi, 0, 256)
        q.product(d[3], x[3], w_hi, b_hi, 0, 256)
        dq, dv = dy(512, "dqk"), dy(256, "dv")
        q.product(dq, x[0], w_in, b_in, 0, 512)                  # the packed in-projection: two row ranges of one gradient
        q.product(dv, x[1], w_in, b_in, 512, 768)
        dn, xn = dy(256, "dn"), FakeTensor((M, 384), name="xn")
        q.product(dn, xn, w_nb, None, 0, 256)                    # no bias gradient with it
        ds, xs = dy(10, "ds"), FakeTensor((M, 256), name="xs")
        q.skinny_product(ds, xs, w_sk)
        q.colsum(ds, b_sk)
        lnp = FakeTensor((2, 256), dtype=torch.float32, name="lnp")
        q.colsum(lnp, gam)
        assert q.first_use(w_hi) and not q.first_use(w_hi) and q.first_use(w_lo) and q.shared_seen == {id(w_hi), id(w_lo)}
        keep = PG.flush_deferred()
        assert (q.products, q.skinny, q.sums, q.shared_seen) == ([], [], [], set())          # empty after a flush
        assert len(keep[0]) == 7 and len(keep[1]) == 2 and len(keep[2]) == 1                 # the operands, for the caller to hold
    names = lambda ts: [t.name for t in ts]                      # noqa: E731
    sk, = [l for l in launches if l[0] == "skinny"]
    assert names(sk[1]) == ["ds"] and names(sk[2]) == ["xs"]
    wg = {(l[1][0].shape[1], l[2][0].shape[1]): l for l in launches if l[0] == "wgrad"}
    assert set(wg) == {(256, 256), (512, 256), (256, 384)}       # one launch per (M, N, K)
    # (256, 256): the lower output first; the shared weight's items in consecutive slots, in insertion order; the in-projection's
    # second half (address 5000 + 512 rows) sorts by its own slice
    g = wg[(256, 256)]
    assert names(g[1]) == ["d1", "dv", "d0", "d2", "d3"] and names(g[2]) == ["x1", "x1", "x0", "x2", "x3"]
    assert names(g[3]) == [("w_lo", 0, 256), ("w_in", 512, 768), ("w_hi", 0, 256), ("w_hi", 0, 256), ("w_hi", 0, 256)]
    assert names(wg[(512, 256)][3]) == [("w_in", 0, 512)] and names(wg[(256, 384)][3]) == [("w_nb", 0, 256)]
    by_out ={tuple(names(l[2])): names(l[1]) for l in launches if l[0] == "colsum"}
    assert by_out == {
        (("b_lo", 0, 256), ("b_in", 512, 768), ("b_hi", 0, 256), ("b_hi", 0, 256), ("b_hi", 0, 256)): ["d1", "dv", "d0", "d2", "d3"],
        (("b_in", 0, 512),): ["dqk"],
        ("b_sk",): ["ds"],                                       # column sums keyed (rows, columns, dtype): the bias of the skinny linear,
        ("gamma",): ["lnp"],                                     # the LayerNorm block partials
        ("w_sk",): [("partial", "ds")],                          # and the skinny product's partials, each a group of its own here
    }
    assert [l[0] for l in launches] == ["skinny"] + ["wgrad"] * 3 + ["colsum"] * 5          # skinny first: its partials join the sums
    assert PG.QUEUE is None and PG.flush_deferred() == ([], [], [])


def test_flush_refuses_a_gradient_it_cannot_write_into(launches):
    d, x = FakeTensor((40, 256)), FakeTensor((40, 256))
    for w, b, text in ((FakeTensor((256, 256)), None, "deferred weight gradient: autograd did not leave a contiguous f32 .grad to write into"),
                       (param((256, 256), 0, "w"), FakeTensor((256,)), "deferred bias gradient: no f32 .grad to write into")):
        with pytest.raises(RuntimeError) as e, PG.deferred_param_grads():
            PG.QUEUE.product(d, x, w, b, 0, 256)
        assert str(e.value) == text and PG.QUEUE is None
    wrong = FakeTensor((128,), grad=FakeTensor((128,), dtype=torch.float32))             # 128 entries for 256 columns
    with pytest.raises(RuntimeError) as e, PG.deferred_param_grads():
        PG.QUEUE.colsum(d, wrong)
    assert str(e.value) == "deferred column sum: no matching contiguous f32 .grad to write into"
    assert launches == []


def test_scope_drops_its_queue_on_an_exception_and_a_nested_scope_restores_the_outer_one(launches):
    w, d, x = param((256, 256), 0, "w"), FakeTensor((40, 256), name="d"), FakeTensor((40, 256), name="x")
    assert PG.QUEUE is None
    with pytest.raises(KeyError):
        with PG.deferred_param_grads():
            dropped = PG.QUEUE
            dropped.product(d, x, w, None, 0, 256)
            dropped.first_use(w)
            raise KeyError("backward failed")
    assert PG.QUEUE is None and launches == []                 # nothing flushed, nothing left behind: shared_seen went with the queue
    with PG.deferred_param_grads():
        outer = PG.QUEUE
        assert outer is not dropped and outer.products == [] and outer.shared_seen == set()
        outer.product(d, x, w, None, 0, 256)
        with PG.deferred_param_grads():
            inner = PG.QUEUE
            assert inner is not outer and inner.products == []
            inner.first_use(w)
        assert PG.QUEUE is outer and len(outer.products) == 1 and outer.shared_seen == set() and launches == []
    assert [l[0] for l in launches] == ["wgrad"] and PG.QUEUE is None
