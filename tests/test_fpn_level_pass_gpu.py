"""GPU: the FPN's level sum as one BatchNorm apply launch forward and one backward (plugin.dense.FUSED_LEVEL_PASS, u3d_bn_apply_sum /
u3d_bn_bwd_apply_sum) against the chain of per-level launches it replaces.  Both are the same element-wise arithmetic with the same
roundings, and the statistics passes are untouched: every result is required to be bit-identical (torch.equal), nothing less.

Shapes: level dims (1,12,20), (1,6,10), (1,3,5) at B = 1 -> 240 output rows.  64 output channels: 32 rows per workgroup pass, 128 per
tile of the new kernels - the last tile is ragged; 256 channels: the benchmark's vector shape (8 rows per pass, 32 per tile).
A width the new kernels refuse must take the chain and give its result: 1024 channels pass the vector-kernel test but their staged
parameters exceed the LDS bound.  (24 channels, which fail the vector-kernel test itself, cannot run as an FPN on the default flags at
all - the chain's own row_map launch refuses them - so that width is checked on the entries' return codes and the route predicate.)"""
import ctypes as C

import pytest
import torch

import projects.mmdet3d_plugin  # noqa: F401
from uni3detr_amd import native as nv
from uni3detr_amd import sparse as sp
from uni3detr_amd.plugin import dense
from uni3detr_amd.plugin.dense import SECOND3DFPN

pytestmark = pytest.mark.gpu

DIMS = [(1, 12, 20), (1, 6, 10), (1, 3, 5)]
CINS = [64, 64, 128]


def _neck(dev, strides, cout):
    L = len(strides)
    g = torch.Generator().manual_seed(11)
    neck = SECOND3DFPN(in_channels=CINS[:L], out_channels=[cout] * L, upsample_strides=strides, use_conv_for_no_stride=True)
    for d in neck.deblocks:
        with torch.no_grad():
            d[0].weight.copy_(torch.randn(d[0].weight.shape, generator=g) * 0.1)
            # both signs of gamma and a bias of the activations' own scale: both ReLU branches occur in every column group
            d[1].weight.copy_((torch.rand(cout, generator=g) + 0.5) * (torch.randint(0, 2, (cout,), generator=g) * 2 - 1))
            d[1].bias.copy_(torch.randn(cout, generator=g) * 0.5)
    xs = [torch.randn((1, CINS[i]) + DIMS[i], generator=g).to(torch.bfloat16) for i in range(L)]
    gout = torch.randn((1, cout) + DIMS[0], generator=g).to(torch.bfloat16)
    return neck.to(dev).train(), [x.to(dev) for x in xs], gout.to(dev)


def _run(dev, strides, cout, level_pass):
    neck, xs, gout = _neck(dev, strides, cout)
    xs = [x.contiguous(memory_format=torch.channels_last_3d).requires_grad_(True) for x in xs]
    old = dense.FUSED_LEVEL_PASS
    dense.FUSED_LEVEL_PASS = level_pass
    try:
        out = neck(xs)
        out.backward(gout.contiguous(memory_format=torch.channels_last_3d))
    finally:
        dense.FUSED_LEVEL_PASS = old
    torch.cuda.synchronize()
    res = {"out": out.detach()}
    for i, x in enumerate(xs):
        res[f"dx{i}"] = x.grad
    for n, p in neck.named_parameters():
        res["grad " + n] = p.grad
    for n, b in neck.named_buffers():
        res["buffer " + n] = b
    return res


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k] is not None and b[k] is not None, k
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("strides,cout", [([1, 2, 4], 64), ([1, 2, 4], 256), ([1, 2], 64), ([1, 2], 256)],
                         ids=["3x64", "3x256", "2x64", "2x256"])
def test_one_pass_is_the_chain_bit_for_bit(cuda, strides, cout, monkeypatch):
    calls = []
    fwd, bwd = nv.bn_apply_sum, nv.bn_bwd_apply_sum
    monkeypatch.setattr(nv, "bn_apply_sum", lambda *a: calls.append("f") or fwd(*a))
    monkeypatch.setattr(nv, "bn_bwd_apply_sum", lambda *a: calls.append("b") or bwd(*a))
    new = _run(cuda, strides, cout, True)
    assert calls == ["f", "b"], "the merged route must have run: one launch forward, one backward"
    chain = _run(cuda, strides, cout, False)
    assert calls == ["f", "b"]
    _same(new, chain)
    out = new["out"].float()
    assert float((out == 0).float().mean()) < 0.9 and all(float(new[f"dx{i}"].float().abs().sum()) > 0 for i in range(len(strides)))
    for i in range(len(strides)):          # every level's running statistics were updated once, on either route
        assert new[f"buffer deblocks.{i}.1.num_batches_tracked"].item() == 1


def test_refused_width_takes_the_chain(cuda, monkeypatch):
    assert not sp.bn_rows_sum_serves(3, 1024, []) and sp.bn_rows_sum_serves(3, 256, []) and not sp.bn_rows_sum_serves(3, 24, [])
    assert not sp.bn_rows_sum_serves(1, 256, []) and not sp.bn_rows_sum_serves(5, 256, [])
    monkeypatch.setattr(nv, "bn_apply_sum", lambda *a: pytest.fail("the merged launch must not be tried"))
    _same(_run(cuda, [1, 2, 4], 1024, True), _run(cuda, [1, 2, 4], 1024, False))


def _arr(ptrs):
    a = (C.c_void_p * len(ptrs))()
    for i, p in enumerate(ptrs):
        a[i] = p
    return a


def test_entry_return_codes(cuda):
    OK, ARG, UNSUPPORTED = 0, -1, nv.U3D_ERR_UNSUPPORTED
    lib = nv.lib()
    c = 64
    x = [torch.zeros((8, c), dtype=torch.bfloat16, device=cuda) for _ in range(3)]
    dx = [torch.zeros_like(t) for t in x]
    par = [[torch.ones(c + 8, dtype=torch.float32, device=cuda) for _ in range(3)] for _ in range(4)]      # mean invstd gamma beta
    sums = [torch.zeros(2 * c + 8, dtype=torch.float64, device=cuda) for _ in range(3)]
    out = torch.full((8, c), 7.0, dtype=torch.bfloat16, device=cuda)
    n_dev = torch.tensor([8], dtype=torch.int32, device=cuda)
    P = lambda ts: _arr([t.data_ptr() for t in ts])
    idx = _arr([None, None, None])

    def fwd(mean=None, xs=None, levels=3, n_cap=8, width=c, dtype=nv.BF16):
        return lib.u3d_bn_apply_sum(xs or P(x), mean or P(par[0]), P(par[1]), P(par[2]), P(par[3]), idx, levels, out.data_ptr(),
                                    n_dev.data_ptr(), n_cap, width, dtype, None)

    def bwd(mean=None, xs=None, levels=3, n_cap=8, width=c, dtype=nv.BF16):
        return lib.u3d_bn_bwd_apply_sum(out.data_ptr(), xs or P(x), mean or P(par[0]), P(par[1]), P(par[2]), P(par[3]), P(sums), idx,
                                        P(dx), levels, n_dev.data_ptr(), n_cap, width, dtype, None)

    odd = _arr([par[0][0].data_ptr(), par[0][1].data_ptr() + 4, par[0][2].data_ptr()])
    null_x = _arr([x[0].data_ptr(), None, x[2].data_ptr()])
    for call in (fwd, bwd):
        assert call(dtype=nv.F32) == UNSUPPORTED                  # bf16 rows only
        assert call(width=24) == UNSUPPORTED                      # 24 % 8 == 0 but 256 % 3 != 0: not a vector-kernel shape
        assert call(width=1024) == UNSUPPORTED                    # the staged parameters of 3 levels exceed the LDS bound
        assert call(mean=odd) == UNSUPPORTED                      # a column parameter off the 16-byte grid
        assert call(xs=null_x) == ARG and call(levels=0) == ARG and call(levels=5) == ARG
        assert call(n_cap=0) == OK                                # no rows: nothing launched
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and all(bool((t == 0).all()) for t in dx), "a refused call must not have launched anything"
