"""GPU parity: HIP geometry + sparse conv + BN + dense vs the CPU oracle (oracle/geometry.py).
Integer results bit-exact (canonical order), fp32 features within 1e-4 relative (MFMA f32 is an exact fma chain;
the difference to torch-CPU is summation order only)."""
import numpy as np
import pytest
import torch

from oracle import geometry as og
from uni3detr_amd import native as nv
from uni3detr_amd.synth import room_scene, uniform_scene, SUNRGBD_RANGE, SUNRGBD_VOXEL

pytestmark = pytest.mark.gpu


def _scenes(n, npts=20000, kind="room"):
    return [room_scene(i, npts)[0] if kind == "room" else uniform_scene(i, npts) for i in range(n)]


def _upload(points_list, dev):
    off = np.cumsum([0] + [p.shape[0] for p in points_list]).astype(np.int32)
    pts = torch.from_numpy(np.concatenate(points_list)).to(dev)
    return pts, torch.from_numpy(off).to(dev)


@pytest.mark.parametrize("kind,npts,max_voxels", [("room", 20000, 16000), ("uniform", 20000, 16000), ("room", 3000, 40000),
                                                  ("room", 20000, 40000)])
def test_voxelize_hard_bit_exact(cuda, kind, npts, max_voxels):
    pl = _scenes(2, npts, kind)
    # ragged: second scene shorter, with out-of-range and NaN points mixed in
    pl[1] = pl[1][: npts - 777].copy()
    pl[1][5, 0] = 100.0
    pl[1][6, 2] = np.nan
    pts, off = _upload(pl, cuda)
    vox, coors, num, mean, voff = nv.voxelize_hard(pts, off, 2, max(p.shape[0] for p in pl), SUNRGBD_VOXEL, SUNRGBD_RANGE, 5,
                                                  max_voxels)
    voff = voff.cpu().numpy()
    rv, rc, rn = og.voxelize_batch(pl, SUNRGBD_VOXEL, SUNRGBD_RANGE, 5, max_voxels)
    assert voff[-1] == rc.shape[0]
    n = int(voff[-1])
    assert np.array_equal(coors[:n].cpu().numpy(), rc)
    assert np.array_equal(num[:n].cpu().numpy(), rn)
    assert np.array_equal(vox[:n].cpu().numpy(), rv)          # exact copies of the kept points
    rm = og.vfe_mean(rv, rn, 4)
    np.testing.assert_allclose(mean[:n].cpu().numpy(), rm, rtol=1e-6, atol=1e-7)


def test_voxelize_empty_scene(cuda):
    pl = [room_scene(0, 500)[0], np.full((10, 4), 50.0, np.float32)]   # second scene entirely out of range
    pts, off = _upload(pl, cuda)
    vox, coors, num, mean, voff = nv.voxelize_hard(pts, off, 2, 500, SUNRGBD_VOXEL, SUNRGBD_RANGE, 5, 16000)
    voff = voff.cpu().numpy()
    rv, rc, rn = og.voxelize_batch(pl, SUNRGBD_VOXEL, SUNRGBD_RANGE, 5, 16000)
    assert voff[2] == voff[1] == rc.shape[0]
    assert np.array_equal(coors[: voff[2]].cpu().numpy(), rc)


def _level0(cuda, batch=2, npts=6000):
    pl = _scenes(batch, npts)
    _, rc, _ = og.voxelize_batch(pl, SUNRGBD_VOXEL, SUNRGBD_RANGE, 5, 16000)
    return rc


def test_bitgrid_rank_and_coords(cuda):
    rc = _level0(cuda)
    dims = (128, 320, 320)
    coors = torch.from_numpy(rc).to(cuda)
    g = nv.BitGrid(2, dims, cuda)
    g.mark(coors)
    g.scan()
    assert int(g.count_dev.item()) == rc.shape[0]
    rank = g.rank(coors).cpu().numpy()
    order = og.block_major_order(rc, dims)
    expect = np.empty_like(order)
    expect[order] = np.arange(order.shape[0])
    assert np.array_equal(rank, expect)
    cc = g.coords(rc.shape[0]).cpu().numpy()
    assert np.array_equal(cc, rc[order])
    # a coordinate that is not occupied ranks -1
    q = torch.tensor([[0, 127, 319, 319], [1, 0, 0, 0], [5, 0, 0, 0]], dtype=torch.int32, device=cuda)
    r2 = g.rank(q).cpu().numpy()
    occupied = {tuple(r) for r in rc.tolist()}
    for row, r in zip(q.cpu().tolist(), r2):
        assert (r >= 0) == (tuple(row) in occupied)


def _canon_table(nbr, q_coors, t_coors):
    """table of indices -> table of partner coordinates keyed by query coordinate (order independent)."""
    K = nbr.shape[0]
    res = {}
    for i, q in enumerate(map(tuple, q_coors.tolist())):
        res[q] = tuple(tuple(t_coors[nbr[k, i]].tolist()) if nbr[k, i] >= 0 else None for k in range(K))
    return res


@pytest.mark.parametrize("pad", [(1, 1, 1), (0, 1, 1)])
def test_rulebook_bit_exact_canonical(cuda, pad):
    rc = _level0(cuda, 2, 3000)
    dims = (128, 320, 320)
    k3, s1, s2, p1 = (3, 3, 3), (1, 1, 1), (2, 2, 2), (1, 1, 1)
    coors = torch.from_numpy(rc).to(cuda)
    g0 = nv.BitGrid(2, dims, cuda)
    g0.mark(coors); g0.scan()
    n0 = rc.shape[0]
    c0 = g0.coords(n0)
    n0_dev = g0.count_dev
    # SubM table
    nbr = g0.nbr_table(c0, n0_dev, k3, s1, p1, 0).cpu().numpy()[:, :n0]
    c0n = c0.cpu().numpy()
    ref = og.nbr_table(c0n, c0n, dims, k3, s1, p1, 0)
    assert np.array_equal(nbr, ref)
    # strided level
    ro, dims1 = og.strided_out_coords(rc, dims, k3, s2, pad)
    g1 = nv.BitGrid(2, dims1, cuda)
    g1.mark_strided(c0, n0_dev, k3, s2, pad); g1.scan()
    n1 = int(g1.count_dev.item())
    assert n1 == ro.shape[0]
    c1 = g1.coords(n1)
    c1n = c1.cpu().numpy()
    assert np.array_equal(c1n[np.lexsort((c1n[:, 3], c1n[:, 2], c1n[:, 1], c1n[:, 0]))], ro)   # same active set
    fwd = g0.nbr_table(c1, g1.count_dev, k3, s2, pad, 0).cpu().numpy()[:, :n1]
    assert np.array_equal(fwd, og.nbr_table(c1n, c0n, dims, k3, s2, pad, 0))
    bwd = g1.nbr_table(c0, n0_dev, k3, s2, pad, 1).cpu().numpy()[:, :n0]
    assert np.array_equal(bwd, og.nbr_table(c0n, c1n, dims1, k3, s2, pad, 1))
    # pair-set symmetry: (i -> o at kappa) in fwd  <=>  (o -> i at kappa) in bwd
    ks, os_ = np.nonzero(fwd >= 0)
    assert np.array_equal(bwd[ks, fwd[ks, os_]], os_)
    assert (fwd >= 0).sum() == (bwd >= 0).sum()


CONV_CASES = [(4, 16, 27), (16, 16, 27), (16, 32, 27), (32, 32, 27), (32, 64, 27), (64, 64, 27), (64, 128, 27),
              (128, 128, 27), (128, 256, 1)]


@pytest.mark.parametrize("cin,cout,kvol", CONV_CASES)
def test_spconv_fwd_bwd_f32(cuda, cin, cout, kvol):
    torch.manual_seed(cin * 1000 + cout)
    rc = _level0(cuda, 2, 2500)
    dims = (128, 320, 320)
    k3, s1, p1 = (3, 3, 3), (1, 1, 1), (1, 1, 1)
    coors = torch.from_numpy(rc).to(cuda)
    g0 = nv.BitGrid(2, dims, cuda)
    g0.mark(coors); g0.scan()
    n = rc.shape[0]
    c0 = g0.coords(n)
    nd = g0.count_dev
    if kvol == 27:
        nbr = g0.nbr_table(c0, nd, k3, s1, p1, 0)
        nbr_t = g0.nbr_table(c0, nd, k3, s1, p1, 1)
        ref_nbr = nbr.cpu().numpy()[:, :n].astype(np.int64)
    else:
        nbr = nbr_t = None
        ref_nbr = np.arange(n, dtype=np.int64)[None]
    x = torch.randn(n, cin)
    w = torch.randn(kvol, cin, cout) * (1.0 / np.sqrt(cin * min(kvol, 9)))
    gy = torch.randn(n, cout)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yr = og.sparse_conv(xr, wr, ref_nbr)
    yr.backward(gy)
    xd, wd, gyd = x.to(cuda), w.to(cuda), gy.to(cuda)
    y = nv.spconv_fwd(xd, wd, nbr, nd, n, cout)
    scale = yr.abs().max().item()
    assert (y.cpu() - yr.detach()).abs().max().item() <= 1e-4 * scale
    dx = nv.spconv_fwd(gyd, wd, nbr_t, nd, n, cin, transpose_w=True)
    assert (dx.cpu() - xr.grad).abs().max().item() <= 1e-4 * xr.grad.abs().max().item()
    dw = nv.spconv_wgrad(xd, gyd, nbr, nd, kvol)
    assert (dw.cpu() - wr.grad).abs().max().item() <= 1e-4 * wr.grad.abs().max().item()


def test_spconv_strided_f32(cuda):
    torch.manual_seed(7)
    rc = _level0(cuda, 2, 2500)
    dims = (128, 320, 320)
    k3, s2, pad = (3, 3, 3), (2, 2, 2), (1, 1, 1)
    coors = torch.from_numpy(rc).to(cuda)
    g0 = nv.BitGrid(2, dims, cuda)
    g0.mark(coors); g0.scan()
    n0 = rc.shape[0]
    c0 = g0.coords(n0)
    dims1 = og.conv_out_dims(dims, k3, s2, pad)
    g1 = nv.BitGrid(2, dims1, cuda)
    g1.mark_strided(c0, g0.count_dev, k3, s2, pad); g1.scan()
    n1 = int(g1.count_dev.item())
    c1 = g1.coords(n1)
    fwd = g0.nbr_table(c1, g1.count_dev, k3, s2, pad, 0)
    bwd = g1.nbr_table(c0, g0.count_dev, k3, s2, pad, 1)
    cin, cout = 16, 32
    x = torch.randn(n0, cin); w = torch.randn(27, cin, cout) * 0.1; gy = torch.randn(n1, cout)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yr = og.sparse_conv(xr, wr, fwd.cpu().numpy()[:, :n1].astype(np.int64))
    yr.backward(gy)
    y = nv.spconv_fwd(x.to(cuda), w.to(cuda), fwd, g1.count_dev, n1, cout)
    assert (y.cpu() - yr.detach()).abs().max().item() <= 1e-4 * yr.abs().max().item()
    dx = nv.spconv_fwd(gy.to(cuda), w.to(cuda), bwd, g0.count_dev, n0, cin, transpose_w=True)
    assert (dx.cpu() - xr.grad).abs().max().item() <= 1e-4 * xr.grad.abs().max().item()
    dw = nv.spconv_wgrad(x.to(cuda), gy.to(cuda), fwd, g1.count_dev, 27)
    assert (dw.cpu() - wr.grad).abs().max().item() <= 1e-4 * wr.grad.abs().max().item()
    # property: equals the dense conv3d restricted to the active output set
    dense = og.dense_conv_reference(x, c0.cpu().numpy(), dims, w, k3, s2, pad, 2)
    c1l = c1.cpu().long()
    sel = dense[c1l[:, 0], :, c1l[:, 1], c1l[:, 2], c1l[:, 3]]
    assert (y.cpu() - sel).abs().max().item() <= 1e-4 * sel.abs().max().item()
    mask = torch.zeros_like(dense[:, 0], dtype=torch.bool)
    mask[c1l[:, 0], c1l[:, 1], c1l[:, 2], c1l[:, 3]] = True
    assert dense.abs().sum(1)[~mask].max().item() == 0.0     # nothing outside the active set


@pytest.mark.parametrize("c,relu,res", [(16, True, False), (64, True, True), (256, True, False), (32, False, False), (20, True, False),
                                        (1024, True, True), (24, True, True)])
def test_bn_fwd_bwd(cuda, c, relu, res):
    torch.manual_seed(c)
    n = 5000
    x = torch.randn(n, c) * 2 + 0.5
    gamma, beta = torch.rand(c) + 0.5, torch.randn(c) * 0.1
    r = torch.randn(n, c) if res else None
    gy = torch.randn(n, c)
    xr = x.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rr = r.clone().requires_grad_(True) if res else None
    yr = og.bn_train(xr, gr, br, 1e-3, rr, relu)
    yr.backward(gy)
    nd = torch.tensor([n], dtype=torch.int32, device=cuda)
    xd = x.to(cuda)
    sums = nv.bn_stats(xd, nd)
    mean = (sums[0] / n)
    var = (sums[1] / n - mean * mean).clamp_min(0)
    np.testing.assert_allclose(mean.cpu().numpy(), x.double().mean(0).numpy(), rtol=1e-6, atol=1e-7)
    invstd = (1.0 / torch.sqrt(var + 1e-3)).float()
    meanf = mean.float()
    # fused statistics + finalisation (what the model calls) == the two-step path, incl. the running-stat update
    rm, rv, nb_t = torch.zeros(c, device=cuda), torch.ones(c, device=cuda), torch.zeros(1, dtype=torch.int64, device=cuda)
    m2, i2 = nv.bn_forward_stats(xd, nd, 1e-3, 0.1, rm, rv, nb_t)
    rm_ref, rv_ref, nb_ref = torch.zeros(c, device=cuda), torch.ones(c, device=cuda), torch.zeros(1, dtype=torch.int64, device=cuda)
    m3, i3 = nv.bn_finalize(sums, nd, n, 1e-3, 0.1, rm_ref, rv_ref, nb_ref)
    assert torch.equal(m2, m3) and torch.equal(i2, i3) and int(nb_t) == 1
    assert torch.allclose(rm, rm_ref, rtol=1e-6, atol=0) and torch.allclose(rv, rv_ref, rtol=1e-6, atol=0)     # fma contraction may differ
    y = nv.bn_apply(xd, meanf, invstd, gamma.to(cuda), beta.to(cuda), r.to(cuda) if res else None, relu, nd)
    assert (y.cpu() - yr.detach()).abs().max().item() <= 2e-5 * max(1.0, yr.abs().max().item())
    gyd = gy.to(cuda)
    bs = nv.bn_bwd_stats(gyd, y, xd, meanf, invstd, relu, nd)
    dx, dres = nv.bn_bwd_apply(gyd, y, xd, meanf, invstd, gamma.to(cuda), bs, relu, nd, res)
    assert (dx.cpu() - xr.grad).abs().max().item() <= 5e-5 * max(1.0, xr.grad.abs().max().item())
    dgamma, dbeta = bs[1].float().cpu(), bs[0].float().cpu()
    np.testing.assert_allclose(dgamma.numpy(), gr.grad.numpy(), rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(dbeta.numpy(), br.grad.numpy(), rtol=1e-4, atol=1e-3)
    if res:
        assert (dres.cpu() - rr.grad).abs().max().item() <= 1e-6
    if relu and not res:
        # mask recomputed from x (y = None) must give the same sums and dx, bit for bit in f32 (same expression as the forward)
        bs2 = nv.bn_bwd_stats(gyd, None, xd, meanf, invstd, relu, nd, gamma.to(cuda), beta.to(cuda))
        dx2, _ = nv.bn_bwd_apply(gyd, None, xd, meanf, invstd, gamma.to(cuda), bs2, relu, nd, False, beta.to(cuda))
        assert torch.equal(bs2, bs) and torch.equal(dx2, dx)
    # bf16 rows against the same f32 reference (vectorized and scalar kernels)
    xb, gb = xd.bfloat16(), gyd.bfloat16()
    rb = r.to(cuda).bfloat16() if res else None
    sb = nv.bn_stats(xb, nd)
    mb = (sb[0] / n).float()
    ib = (1.0 / torch.sqrt((sb[1] / n - (sb[0] / n) ** 2).clamp_min(0) + 1e-3)).float()
    yb = nv.bn_apply(xb, mb, ib, gamma.to(cuda), beta.to(cuda), rb, relu, nd)
    assert (yb.float().cpu() - yr.detach()).abs().max().item() <= 4e-2 * max(1.0, yr.abs().max().item())
    use_y = None if (relu and not res) else yb
    bsb = nv.bn_bwd_stats(gb, use_y, xb, mb, ib, relu, nd, gamma.to(cuda), beta.to(cuda))
    dxb, dresb = nv.bn_bwd_apply(gb, use_y, xb, mb, ib, gamma.to(cuda), bsb, relu, nd, res, beta.to(cuda))
    close = ((dxb.float().cpu() - xr.grad).abs() <= 6e-2 * max(1.0, xr.grad.abs().max().item())).float().mean().item()
    assert close >= 0.995            # a few elements sit on a ReLU edge that bf16 rounding of x flips
    if res:
        assert dresb.dtype == torch.bfloat16


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("c", [64, 256])
def test_bn_mapped_row_order_equals_gather_then_bn(cuda, c, dtype):
    """row_map (u3d_bn_apply / _bwd_stats / _bwd_apply): BatchNorm that writes row r of x to row row_map[r] of y == a row gather
    followed by BatchNorm, forward and backward, bit for bit in the outputs (same per-row arithmetic; the f64 column sums only
    differ in summation order)."""
    from uni3detr_amd import sparse as sp
    torch.manual_seed(c)
    n = 4096 + 128
    x = (torch.randn(n, c, device=cuda) * 1.5 + 0.3).to(dtype)
    perm = torch.randperm(n, device=cuda)                     # idx: output row -> source row
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(n, device=cuda)
    idx32, inv32 = perm.int().contiguous(), inv.int().contiguous()
    nd = torch.tensor([n], dtype=torch.int32, device=cuda)
    gy = torch.randn(n, c, device=cuda).to(dtype)
    outs = []
    for mapped in (False, True):
        torch.manual_seed(1)                                      # same affine parameters in both runs
        bn = torch.nn.BatchNorm1d(c, eps=1e-3, momentum=0.01).to(cuda).train()
        with torch.no_grad():
            bn.weight.copy_(torch.rand(c, device=cuda) + 0.5); bn.bias.copy_(torch.randn(c, device=cuda) * 0.1)
        xr = x.clone().requires_grad_(True)
        if mapped:
            y = sp.bn_rows(xr, bn, nd, None, True, row_map=inv32)
            y.backward(gy)
            dx = xr.grad
        else:
            xg = nv.gather_rows(x, idx32).requires_grad_(True)
            y = sp.bn_rows(xg, bn, nd, None, True)
            y.backward(gy)
            dx = nv.gather_rows(xg.grad, inv32)               # back to the source row order
        outs.append((y.detach(), dx, bn.weight.grad.clone(), bn.bias.grad.clone(), bn.running_mean.clone(), bn.running_var.clone()))
    (y0, dx0, gw0, gb0, rm0, rv0), (y1, dx1, gw1, gb1, rm1, rv1) = outs
    assert torch.allclose(rm0, rm1, rtol=1e-6, atol=1e-7) and torch.allclose(rv0, rv1, rtol=1e-6, atol=1e-7)
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    assert (y0.float() - y1.float()).abs().max().item() <= tol * max(1.0, y0.float().abs().max().item())
    assert (dx0.float() - dx1.float()).abs().max().item() <= tol * max(1.0, dx0.float().abs().max().item())
    assert torch.allclose(gw0, gw1, rtol=1e-4, atol=1e-3) and torch.allclose(gb0, gb1, rtol=1e-4, atol=1e-3)


def test_dense_roundtrip(cuda):
    rc = _level0(cuda, 2, 1500)
    dims = (15, 40, 40)
    rng = np.random.default_rng(0)
    cells = rng.choice(2 * 15 * 40 * 40, 3000, replace=False)
    co = np.stack([cells // (15 * 1600), cells // 1600 % 15, cells // 40 % 40, cells % 40], 1).astype(np.int32)
    f = torch.randn(3000, 256)
    nd = torch.tensor([3000], dtype=torch.int32, device=cuda)
    vol = nv.to_dense(f.to(cuda), torch.from_numpy(co).to(cuda), nd, 2, dims)
    ref = og.to_dense(f, co, 2, dims)
    assert vol.shape == ref.shape and torch.equal(vol.cpu(), ref)
    back = nv.from_dense(vol.permute(0, 2, 3, 4, 1).contiguous(), torch.from_numpy(co).to(cuda), nd, 3000)
    assert torch.equal(back.cpu(), f)


BF16_CASES = [(8, 16, 27), (16, 32, 27), (32, 64, 27), (64, 64, 27), (64, 128, 27), (128, 128, 27), (128, 256, 1), (256, 256, 27),
              (256, 128, 27), (512, 512, 1), (128, 64, 27), (64, 32, 27), (64, 16, 27)]


@pytest.mark.parametrize("v2", [True, False])
@pytest.mark.parametrize("cin,cout,kvol", BF16_CASES)
def test_spconv_fwd_bwd_bf16(cuda, cin, cout, kvol, v2):
    """bf16 operands / f32 accumulation, both kernel generations, against the f32 oracle on bf16-rounded inputs."""
    torch.manual_seed(cin * 1000 + cout + 7)
    rc = _level0(cuda, 2, 2500)
    dims = (128, 320, 320)
    k3, s1, p1 = (3, 3, 3), (1, 1, 1), (1, 1, 1)
    coors = torch.from_numpy(rc).to(cuda)
    g0 = nv.BitGrid(2, dims, cuda)
    g0.mark(coors); g0.scan()
    n = rc.shape[0]
    c0 = g0.coords(n)
    nd = g0.count_dev
    if kvol == 27:
        nbr = g0.nbr_table(c0, nd, k3, s1, p1, 0)
        nbr_t = g0.nbr_table(c0, nd, k3, s1, p1, 1)
        ref_nbr = nbr.cpu().numpy()[:, :n].astype(np.int64)
    else:
        nbr = nbr_t = None
        ref_nbr = np.arange(n, dtype=np.int64)[None]
    x = torch.randn(n, cin).bfloat16().float()
    w = (torch.randn(kvol, cin, cout) * (1.0 / np.sqrt(cin * min(kvol, 9)))).bfloat16().float()
    gy = torch.randn(n, cout).bfloat16().float()
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yr = og.sparse_conv(xr, wr, ref_nbr)
    yr.backward(gy)
    old = nv.USE_IGEMM_V2
    nv.USE_IGEMM_V2 = v2
    try:
        xd, wd, gyd = x.to(cuda).bfloat16(), w.to(cuda).bfloat16(), gy.to(cuda).bfloat16()
        y = nv.spconv_fwd(xd, wd, nbr, nd, n, cout)
        dx = nv.spconv_fwd(gyd, wd, nbr_t, nd, n, cin, transpose_w=True)
        dw = nv.spconv_wgrad(xd, gyd, nbr, nd, kvol)
        # n-major weights ([K, Cout, Cin]): the LDS-DMA forward the model uses must give the k-major kernel's result
        y_nm = nv.spconv_fwd(xd, wd.transpose(1, 2).contiguous(), nbr, nd, n, cout, transpose_w=True)
        # capacity mode: buffers larger than the device-side row count; rows past the count are never produced from
        cap = n + 777
        xpad = torch.cat([xd, torch.full((cap - n, cin), float("nan"), device=cuda, dtype=torch.bfloat16)])
        gpad = torch.cat([gyd, torch.full((cap - n, cout), float("nan"), device=cuda, dtype=torch.bfloat16)])
        nbr_c = nbr_tc = None
        if nbr is not None:
            nbr_c = torch.full((kvol, (cap + 127) // 128 * 128), -1, dtype=torch.int32, device=cuda)
            nbr_tc = nbr_c.clone()
            nbr_c[:, :n] = nbr[:, :n]
            nbr_tc[:, :n] = nbr_t[:, :n]
        y_cap = nv.spconv_fwd(xpad, wd, nbr_c, nd, cap, cout)
        dx_cap = nv.spconv_fwd(gpad, wd, nbr_tc, nd, cap, cin, transpose_w=True)
        dw_cap = nv.spconv_wgrad(xpad, gpad, nbr_c, nd, kvol)
        zero = torch.zeros(1, dtype=torch.int32, device=cuda)
        dw_zero = nv.spconv_wgrad(xpad, gpad, nbr_c, zero, kvol)
    finally:
        nv.USE_IGEMM_V2 = old
    assert (y_nm.float() - y.float()).abs().max().item() <= 1e-2 * yr.abs().max().item()
    assert torch.equal(y_cap[:n], y) and torch.equal(dx_cap[:n], dx)
    # the row split of the weight gradient follows the capacity: same terms, different f32 summation order (and no NaN leaked in)
    assert (dw_cap - dw).abs().max().item() <= 1e-4 * max(1.0, dw.abs().max().item())
    assert float(dw_zero.abs().max()) == 0.0
    assert (y.float().cpu() - yr.detach()).abs().max().item() <= 1e-2 * yr.abs().max().item()          # bf16 output rounding
    assert (dx.float().cpu() - xr.grad).abs().max().item() <= 1e-2 * xr.grad.abs().max().item()
    assert (dw.cpu() - wr.grad).abs().max().item() <= 2e-3 * wr.grad.abs().max().item()                 # f32 accumulate, f32 output


def test_dense_lattice_conv_matches_conv3d(cuda):
    """A dense volume is the all-active special case: conv on the lattice table == F.conv3d (zero padding), incl. strides."""
    import torch.nn.functional as F
    from uni3detr_amd.plugin import dense as dn
    from uni3detr_amd import sparse as sp
    torch.manual_seed(3)
    B, C, D, H, W = 2, 64, 5, 12, 10
    x = torch.randn(B, C, D, H, W)
    for (k, s, p, co) in [((1, 3, 3), (1, 1, 1), (0, 1, 1), 64), ((1, 3, 3), (1, 2, 2), (0, 1, 1), 128), ((3, 3, 3), (1, 1, 1), (1, 1, 1), 64),
                          ((1, 1, 1), (1, 1, 1), (0, 0, 0), 128)]:
        w = torch.randn(co, C, *k) * 0.05
        gy = None
        xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        ref = F.conv3d(xr, wr, None, s, p)
        gy = torch.randn_like(ref)
        ref.backward(gy)
        rows = x.permute(0, 2, 3, 4, 1).reshape(-1, C).contiguous().to(cuda).requires_grad_(True)
        wd = w.to(cuda).requires_grad_(True)
        geom, dims_out = dn.Lattice.conv(cuda, B, (D, H, W), k, s, p)
        y = sp.sparse_conv(rows, wd.permute(2, 3, 4, 1, 0), geom)
        assert dims_out == tuple(ref.shape[2:])
        yv = y.view(B, *dims_out, co).permute(0, 4, 1, 2, 3)
        assert (yv.detach().cpu() - ref.detach()).abs().max().item() <= 1e-4 * ref.abs().max().item()
        y.backward(gy.permute(0, 2, 3, 4, 1).reshape(-1, co).contiguous().to(cuda))
        gx = rows.grad.view(B, D, H, W, C).permute(0, 4, 1, 2, 3).cpu()
        assert (gx - xr.grad).abs().max().item() <= 1e-4 * xr.grad.abs().max().item()
        assert (wd.grad.cpu() - wr.grad).abs().max().item() <= 1e-4 * wr.grad.abs().max().item()
    # (1,s,s) transposed conv == ConvTranspose3d
    for s in (2, 4):
        dec = torch.nn.ConvTranspose3d(C, 32, (1, s, s), stride=(1, s, s), bias=False)
        bn = torch.nn.BatchNorm3d(32, eps=1e-3, momentum=0.01)
        ref = F.relu(bn(dec(x)))
        dec_d, bn_d = torch.nn.ConvTranspose3d(C, 32, (1, s, s), stride=(1, s, s), bias=False).to(cuda), torch.nn.BatchNorm3d(32, eps=1e-3, momentum=0.01).to(cuda)
        dec_d.load_state_dict(dec.state_dict())
        rows = x.permute(0, 2, 3, 4, 1).reshape(-1, C).contiguous().to(cuda)
        y, dims_out = dn.deconv_bn_relu(rows, B, (D, H, W), dec_d, bn_d)
        yv = y.view(B, *dims_out, 32).permute(0, 4, 1, 2, 3)
        assert (yv.detach().cpu() - ref.detach()).abs().max().item() <= 1e-4 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("stride,cout", [((1, 2, 2), 128), ((1, 4, 4), 256), ((2, 2, 2), 64)])
def test_strided_dgrad_split_path_matches_conv3d(cuda, stride, cout):
    """bf16 input gradient of a strided lattice conv through (per-offset GEMM over output rows + u3d_tap_gather_sum) equals the
    output-stationary dgrad kernel and F.conv3d's input gradient."""
    import torch.nn.functional as F
    from uni3detr_amd.plugin import dense as dn
    from uni3detr_amd import sparse as sp
    torch.manual_seed(11)
    B, C, D, H, W = 2, 64, 6, 16, 12
    k = (3, 3, 3) if stride[0] > 1 else (1, 3, 3)
    p = (1, 1, 1) if stride[0] > 1 else (0, 1, 1)
    x = torch.randn(B, C, D, H, W).bfloat16().float()
    w = (torch.randn(cout, C, *k) * 0.05).bfloat16().float()
    xr = x.clone().requires_grad_(True)
    ref = F.conv3d(xr, w, None, stride, p)
    gy = torch.randn_like(ref).bfloat16().float()
    ref.backward(gy)
    geom, dims_out = dn.Lattice.conv(cuda, B, (D, H, W), k, stride, p)
    assert geom.strided
    got = {}
    for split in (True, False):
        sp.STRIDED_DGRAD_SPLIT = split
        try:
            rows = x.permute(0, 2, 3, 4, 1).reshape(-1, C).contiguous().to(cuda).bfloat16().requires_grad_(True)
            y = sp.sparse_conv(rows, w.to(cuda).permute(2, 3, 4, 1, 0).contiguous(), geom)
            y.backward(gy.permute(0, 2, 3, 4, 1).reshape(-1, cout).contiguous().to(cuda).bfloat16())
            got[split] = rows.grad.float().view(B, D, H, W, C).permute(0, 4, 1, 2, 3).cpu()
        finally:
            sp.STRIDED_DGRAD_SPLIT = True
    # nn.Conv3d-layout parameter ("oidhw"): the bf16 weight gradient comes back in the parameter's own layout
    wr = w.clone().requires_grad_(True)
    F.conv3d(x, wr, None, stride, p).backward(gy)
    wp = torch.nn.Parameter(w.to(cuda))
    rows = x.permute(0, 2, 3, 4, 1).reshape(-1, C).contiguous().to(cuda).bfloat16()
    sp.sparse_conv(rows, wp, geom, "oidhw").backward(gy.permute(0, 2, 3, 4, 1).reshape(-1, cout).contiguous().to(cuda).bfloat16())
    assert wp.grad.shape == wp.shape and wp.grad.is_contiguous()
    assert (wp.grad.cpu() - wr.grad).abs().max().item() <= 2e-2 * wr.grad.abs().max().item()
    scale = xr.grad.abs().max().item()
    assert (got[True] - xr.grad).abs().max().item() <= 2e-2 * scale
    assert (got[False] - xr.grad).abs().max().item() <= 2e-2 * scale
    assert (got[True] - got[False]).abs().max().item() <= 2e-2 * scale


@pytest.mark.parametrize("cin,cout,B,dims", [(64, 64, 2, (5, 12, 10)), (128, 256, 3, (4, 11, 9)), (256, 256, 8, (15, 40, 40)),
                                             (32, 32, 3, (7, 13, 11)), (16, 32, 2, (5, 12, 10)), (64, 32, 2, (6, 9, 14)), (32, 16, 4, (9, 20, 17)),
                                             (64, 16, 1, (3, 5, 4)), (512, 512, 8, (15, 10, 10)),
                                             # 192-row tiles of the eight-phase kernels: a partial last tile; and a shape BOTH wide-tile rules accept, where
                                             # the 256-column kernel (dispatched) and the 128-column one would choose different tile heights - the
                                             # statistics buffer must be sized by the dispatched kernel's (u3d_igemm_fwd_stats_rows)
                                             (256, 256, 3, (15, 32, 31)), (512, 512, 10, (10, 20, 20))])
def test_conv_epilogue_bn_statistics_match_separate_pass(cuda, cin, cout, B, dims):
    """conv -> BatchNorm with the statistics reduced in the conv epilogue (u3d_igemm_fwd_bf16 with stats + u3d_bn_finalize_partials) equals
    the conv followed by the stand-alone statistics pass: outputs, running statistics, and the backward through both."""
    from uni3detr_amd.plugin import dense as dn
    from uni3detr_amd import sparse as sp
    torch.manual_seed(cin + cout)
    D, H, W = dims
    k, s_, p = (3, 3, 3), (1, 1, 1), (1, 1, 1)
    geom, _ = dn.Lattice.conv(cuda, B, dims, k, s_, p)
    n = B * D * H * W
    x = torch.randn(n, cin, device=cuda).bfloat16()
    w = torch.nn.Parameter((torch.randn(*k, cin, cout, device=cuda) * 0.05))
    gy = torch.randn(n, cout, device=cuda).bfloat16()
    res = {}
    for fused in (True, False):
        sp.FUSED_CONV_STATS = fused
        try:
            bn = torch.nn.BatchNorm1d(cout, eps=1e-3, momentum=0.01).to(cuda).train()
            with torch.no_grad():
                bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.1)
            torch.manual_seed(1)
            with torch.no_grad():
                bn.weight.copy_(torch.linspace(0.5, 1.5, cout)); bn.bias.copy_(torch.linspace(-0.2, 0.2, cout))
            xq = x.clone().requires_grad_(True)
            w.grad = None
            y = sp.conv_bn(xq, w, geom, bn, geom.n_out_dev, None, True)
            y.backward(gy)
            res[fused] = (y.detach().float(), bn.running_mean.clone(), bn.running_var.clone(), xq.grad.float(), w.grad.clone(), bn.weight.grad.clone())
        finally:
            sp.FUSED_CONV_STATS = True
    a, b = res[True], res[False]
    assert (a[0] - b[0]).abs().max().item() <= 2e-2 * max(1.0, b[0].abs().max().item())
    assert torch.allclose(a[1], b[1], rtol=1e-4, atol=1e-6) and torch.allclose(a[2], b[2], rtol=1e-4, atol=1e-6)
    for i in (3, 4, 5):
        assert (a[i] - b[i]).abs().max().item() <= 3e-2 * max(1e-3, b[i].abs().max().item()), i


def test_dynamic_voxelize_and_scatter_mean(cuda):
    from uni3detr_amd.plugin.detector import DynamicSimpleVFE
    rng = np.random.default_rng(2)
    rangep = (-6.4, -6.4, -0.1, 6.4, 6.4, 2.46)
    pl = []
    for b in range(2):
        p = room_scene(b, 30000 - 5000 * b)[0].copy()
        p[:, :2] *= 1.5
        p[:, 2] += 2.0
        p[:50] += 100.0                                     # out-of-range points -> -1 rows
        pl.append(p)
    pts, off = _upload(pl, cuda)
    coors = nv.voxelize_dynamic(pts, off, 2, SUNRGBD_VOXEL, rangep)
    rc, rfeat, rvox = og.voxelize_dynamic(pl, SUNRGBD_VOXEL, rangep)
    assert np.array_equal(coors.cpu().numpy(), rc)
    vfe = DynamicSimpleVFE(SUNRGBD_VOXEL, rangep)
    feats, fcoors = vfe(pts, coors, batch_size=2)
    assert np.array_equal(fcoors.cpu().numpy(), rvox)                  # lexicographic order == torch.unique(dim=0)
    np.testing.assert_allclose(feats.cpu().numpy(), rfeat, rtol=1e-5, atol=1e-5)


def test_full_size_dominant_layer_properties(cuda):
    """The layer `roofline` reports on, at BASELINE.json's full size (8 scenes: 192 000 lattice rows, 256 -> 256 channels, 3x3x3),
    through the kernels the step uses (n-major forward + epilogue statistics, dgrad, weight gradient): size-independent properties
    instead of a full oracle run -
      * forward rows sampled all over the tensor (first / middle / last tiles) == f32 gather-GEMM of the same bf16 operands,
      * the epilogue's BatchNorm statistics == column sums / sums of squares of the output it wrote,
      * adjointness <conv(x), dy> == <x, dgrad(dy)> == <W, wgrad(x, dy)>  (one scalar ties the three kernels together),
      * linearity conv(x1 + x2) == conv(x1) + conv(x2) up to bf16 output rounding."""
    torch.manual_seed(3)
    B, dims, C, ks = 8, (15, 40, 40), 256, (3, 3, 3)
    n = B * dims[0] * dims[1] * dims[2]
    nbr = nv.dense_nbr_table(B, dims, dims, ks, (1, 1, 1), (1, 1, 1), 0, cuda)
    nbr_b = nv.dense_nbr_table(B, dims, dims, ks, (1, 1, 1), (1, 1, 1), 1, cuda)
    nd = nv.count_tensor(n, cuda)
    x = (torch.randn(n, C, device=cuda) * 0.5).bfloat16()
    dy = (torch.randn(n, C, device=cuda) * 0.5).bfloat16()
    w = (torch.randn(27, C, C, device=cuda) * 0.03).bfloat16()            # kio [K, Cin, Cout]
    koi = w.transpose(1, 2).contiguous()                                  # n-major for the forward kernel
    y, stats, tile_rows = nv.spconv_fwd(x, koi, nbr, nd, n, C, transpose_w=True, tag="spconv_fwd", want_stats=True)
    assert stats is not None
    # (1) sampled rows vs f32 gather-GEMM
    rows = torch.cat([torch.arange(0, 300, device=cuda), torch.arange(n // 2 - 150, n // 2 + 150, device=cuda), torch.arange(n - 300, n, device=cuda)])
    exp = torch.zeros(rows.numel(), C, device=cuda)
    xf = torch.cat([x.float(), torch.zeros(1, C, device=cuda)])
    for k in range(27):
        idx = nbr[k, rows].long()
        idx = torch.where(idx < 0, torch.full_like(idx, n), idx)
        exp += xf[idx] @ w[k].float()
    got = y[rows].float()
    assert (got - exp).abs().max().item() <= 1.5e-2 * exp.abs().max().item()
    # (2) epilogue statistics vs the stored output (f32 accumulators in the kernel, bf16-rounded output: loose on the squares)
    yf = y.float()
    s0, s1 = stats[:, 0].sum(0), stats[:, 1].sum(0)
    assert stats.shape == ((n + tile_rows - 1) // tile_rows, 2, C)
    assert torch.allclose(s0.float(), yf.sum(0), rtol=2e-2, atol=2.0)
    assert torch.allclose(s1.float(), (yf * yf).sum(0), rtol=2e-2)
    # (3) adjointness across the three kernels
    dx = nv.spconv_fwd(dy, w, nbr_b, nd, n, C, transpose_w=True)
    dw = nv.spconv_wgrad(x, dy, nbr, nd, 27)
    a = (yf.double() * dy.double()).sum().item()
    b = (x.double() * dx.double()).sum().item()
    c = (w.double() * dw.double()).sum().item()
    # y and dx are stored in bf16 (relative rounding 2^-9, random sign): the three sums of ~49 M zero-mean terms agree up to that
    # rounding noise, whose scale is the root of the summed squares - not the (tiny) net sum
    noise = ((yf.double() * dy.double()).pow(2).sum() + (x.double() * dx.double()).pow(2).sum()).sqrt().item()
    assert abs(a - b) <= 1.5e-2 * noise and abs(a - c) <= 1.5e-2 * noise and abs(b - c) <= 1.5e-2 * noise, (a, b, c, noise)
    # (4) linearity
    x2 = (torch.randn(n, C, device=cuda) * 0.5).bfloat16()
    xs = (x.float() + x2.float()).bfloat16()
    y2 = nv.spconv_fwd(x2, koi, nbr, nd, n, C, transpose_w=True, tag="spconv_fwd")
    ys = nv.spconv_fwd(xs, koi, nbr, nd, n, C, transpose_w=True, tag="spconv_fwd")
    lin = (ys.float() - (yf + y2.float()))[rows]
    assert lin.abs().max().item() <= 4e-2 * ys.float().abs().max().item()


def test_subm_transposed_table_is_the_reversed_forward_table(cuda):
    """native.RevNbr: the input gradient of a SubM layer reads the forward table with the 27 offsets reversed instead of building
    the transposed table (sparse.Level.subm_tables).  Pinned here against the table the builder produces in transposed mode, on a
    ragged multi-scene level, and through the dgrad itself (bf16 direct kernel + f32 first-generation kernel)."""
    import torch
    from uni3detr_amd import native as nv
    from uni3detr_amd import sparse as sp
    torch.manual_seed(3)
    dims = (16, 40, 36)
    coors = torch.unique(torch.stack([torch.randint(0, 3, (6000,)), torch.randint(0, dims[0], (6000,)), torch.randint(0, dims[1], (6000,)),
                                      torch.randint(0, dims[2], (6000,))], 1), dim=0).int().cuda()
    lvl, _ = sp.level_from_coors(coors, 3, dims)
    fwd = lvl.grid.nbr_table(lvl.coords, lvl.n_dev, sp.K3, sp.S1, sp.P1, 0)
    bwd = lvl.grid.nbr_table(lvl.coords, lvl.n_dev, sp.K3, sp.S1, sp.P1, 1)
    assert torch.equal(bwd[:, :lvl.n], fwd.flip(0)[:, :lvl.n])
    for dt, cin, cout in ((torch.bfloat16, 32, 32), (torch.bfloat16, 64, 64), (torch.float32, 16, 16)):
        dy = torch.randn(lvl.n, cout, device="cuda").to(dt)
        w = (torch.randn(27, cin, cout, device="cuda") * 0.1).to(dt)
        a = nv.spconv_fwd(dy, w, bwd, lvl.n_dev, lvl.n, cin, transpose_w=True)
        b = nv.spconv_fwd(dy, w, nv.RevNbr(fwd), lvl.n_dev, lvl.n, cin, transpose_w=True)
        assert torch.equal(a, b), (dt, cin, cout)


def _level(seed=5, n_pts=9000, batch=3, dims=(16, 40, 36)):
    import torch
    from uni3detr_amd import sparse as sp
    torch.manual_seed(seed)
    coors = torch.unique(torch.stack([torch.randint(0, batch, (n_pts,)), torch.randint(0, dims[0], (n_pts,)),
                                      torch.randint(0, dims[1], (n_pts,)), torch.randint(0, dims[2], (n_pts,))], 1), dim=0).int().cuda()
    lvl, _ = sp.level_from_coors(coors, batch, dims)
    return lvl, lvl.grid.nbr_table(lvl.coords, lvl.n_dev, sp.K3, sp.S1, sp.P1, 0)


def _ref_conv(x, w, nbr, n):
    import torch
    out = torch.zeros(n, w.shape[2], dtype=torch.float32, device=x.device)
    xf = torch.cat([x.float(), torch.zeros(1, x.shape[1], device=x.device)])
    for k in range(w.shape[0]):
        idx = nbr[k, :n].long()
        idx = torch.where(idx < 0, torch.full_like(idx, x.shape[0]), idx)
        out += xf[idx] @ w[k].float()
    return out


@pytest.mark.parametrize("cin,cout", [(16, 16), (16, 32), (32, 32), (32, 64)])
def test_narrow_weight_gradient_kernel_matches_f32_reference(cuda, cin, cout):
    """wgrad_narrow.hip (9 waves x 3 offsets, stationary dout tile): every offset's dW against an f32 gather-matmul, both output
    layouts, with a device-side row count BELOW the capacity (rows past it hold garbage and must not be read as data) and with zero rows."""
    import torch
    from uni3detr_amd import native as nv
    lvl, nbr = _level()
    n = lvl.n
    torch.manual_seed(cin + cout)
    x = torch.randn(n, cin, device="cuda").bfloat16()
    dy = torch.randn(n, cout, device="cuda").bfloat16()
    xf = torch.cat([x.float(), torch.zeros(1, cin, device="cuda")])
    exp = []
    for k in range(27):
        idx = nbr[k, :n].long()
        idx = torch.where(idx < 0, torch.full_like(idx, n), idx)
        exp.append(xf[idx].t() @ dy.float())
    exp = torch.stack(exp)                                                       # [27, cin, cout]
    got = nv.spconv_wgrad(x, dy, nbr, lvl.n_dev, 27)
    scale = exp.abs().max()
    assert (got - exp).abs().max() / scale < 2e-5                                # bf16 products are exact in f32; only the summation order differs
    got_oik = nv.spconv_wgrad(x, dy, nbr, lvl.n_dev, 27, out_oik=True)
    assert torch.equal(got_oik, got.permute(2, 1, 0).contiguous())
    # fewer live rows than the tensors hold: NaN in the dead rows must not reach the result
    m = n - 777
    cnt = nv.count_tensor(m, x.device)
    x2, dy2 = x.clone(), dy.clone()
    x2[m:] = float("nan"); dy2[m:] = float("nan")
    nb2 = nbr.clone()
    nb2[:, :m][nb2[:, :m] >= m] = -1                                             # a live row never points at a dead one in the real tables
    exp2 = torch.stack([torch.cat([x2[:m].float(), torch.zeros(1, cin, device="cuda")])[torch.where(nb2[k, :m] < 0, torch.full_like(nb2[k, :m], m), nb2[k, :m]).long()].t()
                        @ dy2[:m].float() for k in range(27)])
    got2 = nv.spconv_wgrad(x2, dy2, nb2, cnt, 27)
    assert torch.isfinite(got2).all() and (got2 - exp2).abs().max() / exp2.abs().max() < 2e-5
    assert (nv.spconv_wgrad(x, dy, nbr, nv.count_tensor(0, x.device), 27) == 0).all()
    assert torch.equal(nv.spconv_wgrad(x, dy, nbr, lvl.n_dev, 27), got)         # deterministic


@pytest.mark.parametrize("cin,cout", [(32, 32), (16, 32), (64, 32), (64, 64), (128, 128)])
def test_input_gradient_with_addend_epilogue(cuda, cin, cout):
    """u3d_igemm_fwd_bf16 with an addend (direct-operand kernels and the 128-row LDS-DMA tiles): conv + addend rounded once == f32 reference."""
    import torch
    from uni3detr_amd import native as nv
    lvl, nbr = _level(seed=9)
    n = lvl.n
    torch.manual_seed(cin * 3 + cout)
    dy = torch.randn(n, cin, device="cuda").bfloat16()
    w = (torch.randn(27, cout, cin, device="cuda") * 0.1).bfloat16()           # n-major [K][Cout_gemm][Cin_gemm] as the dgrad passes it
    add = torch.randn(n, cout, device="cuda").bfloat16()
    got = nv.spconv_fwd(dy, w, nbr, lvl.n_dev, n, cout, transpose_w=True, addend=add).float()
    exp = _ref_conv(dy, w.transpose(1, 2), nbr, n) + add.float()
    assert (got - exp).abs().max() / exp.abs().max() < 1e-2
    plain = nv.spconv_fwd(dy, w, nbr, lvl.n_dev, n, cout, transpose_w=True).float()
    assert ((plain + add.float()) - got).abs().max() / exp.abs().max() < 1.6e-2   # the two-pass form rounds twice


def test_skinny_weight_gradients_batched_equal_single_launches(cuda):
    import torch
    from uni3detr_amd import native as nv
    torch.manual_seed(0)
    m = 7200
    shapes = [(8, 256), (10, 256), (1, 256), (1, 256), (256, 3), (256, 3)]
    dys = [torch.randn(m, n, device="cuda").bfloat16() for n, _ in shapes]
    xs = [torch.randn(m, k, device="cuda").bfloat16() for _, k in shapes]
    parts = nv.skinny_wgrad_partial_batched(dys, xs)
    for d, x, p in zip(dys, xs, parts):
        assert torch.equal(p, nv.skinny_wgrad_partial(d, x))
        dw = p.sum(0).view(d.shape[1], x.shape[1])
        ref = d.float().t() @ x.float()
        assert (dw - ref).abs().max() / ref.abs().max() < 1e-4


def test_conv_weight_gradient_in_flat_view_and_shared_weight(cuda):
    """TrainStep hands every parameter a view of the flat gradient buffer (`_u3d_grad_view`): a conv writes its weight gradient
    there in place when the weight is used ONCE in the step; a weight used twice must fall back to fresh tensors (autograd adds them)."""
    import torch
    from uni3detr_amd import sparse as sp
    lvl, _ = _level(seed=11, n_pts=4000)
    geom = sp.subm_geom(lvl)
    torch.manual_seed(1)
    x = torch.randn(lvl.n, 32, device="cuda").bfloat16().requires_grad_(True)
    w = torch.nn.Parameter(torch.randn(3, 3, 3, 32, 32, device="cuda") * 0.05)
    flat = torch.zeros(w.numel() + 64, device="cuda")
    w._u3d_grad_view = flat[64:].view_as(w)
    # single use: the gradient IS the view
    sp.reset_conv_uses()
    y = sp.sparse_conv(x, w, geom)
    y.float().square().sum().backward()
    assert w.grad.data_ptr() == w._u3d_grad_view.data_ptr()
    g1 = w.grad.clone()
    assert torch.equal(flat[64:].view_as(w), g1) and (flat[:64] == 0).all()
    # two uses in one step: grad = sum of both, not an aliased overwrite
    w.grad = None; x.grad = None
    flat.zero_()
    sp.reset_conv_uses()
    y2 = sp.sparse_conv(sp.sparse_conv(x, w, geom), w, geom)
    y2.float().square().sum().backward()
    got = w.grad.clone()
    w.grad = None; x.grad = None
    del w._u3d_grad_view
    sp.reset_conv_uses()
    y3 = sp.sparse_conv(sp.sparse_conv(x, w, geom), w, geom)
    y3.float().square().sum().backward()
    assert torch.equal(got, w.grad)


def test_eight_phase_kernels_against_the_128_tile_kernels_and_stable_under_load(cuda):
    """The 256 x 256 eight-phase kernel (counted vmcnt, raw barriers, wave rows one barrier apart: a schedule whose failure mode is a RARE
    stale tile) against the 128 x 128-tile kernel with its one __syncthreads() per k-tile, at the full size of the dominant layer and on a
    ragged row count: both feed the MFMAs the same k-groups in the same order, so every element must be BIT-identical - any tile read
    before its LDS-DMA landed shows up as a difference.  Then 24 more launches while a second stream saturates HBM (load latencies move):
    every result equal to the first."""
    torch.manual_seed(11)
    B, dims, C, ks = 8, (15, 40, 40), 256, (3, 3, 3)
    n_full = B * dims[0] * dims[1] * dims[2]
    nbr = nv.dense_nbr_table(B, dims, dims, ks, (1, 1, 1), (1, 1, 1), 0, cuda)
    x = (torch.randn(n_full, C, device=cuda) * 0.5).bfloat16()
    koi = (torch.randn(27, C, C, device=cuda) * 0.03).bfloat16()          # n-major [K][Cout][Cin]
    halves = [koi[:, :128].contiguous(), koi[:, 128:].contiguous()]       # Cout = 128: served by the 128 x 128 tiles
    for n in (n_full, n_full - 4321):                                     # the second: a partial last tile, rows past n never written
        nd = nv.count_tensor(n, cuda)
        y = nv.spconv_fwd(x, koi, nbr, nd, n_full, C, transpose_w=True, tag="spconv_fwd")
        lo = nv.spconv_fwd(x, halves[0], nbr, nd, n_full, 128, transpose_w=True, tag="spconv_fwd")
        hi = nv.spconv_fwd(x, halves[1], nbr, nd, n_full, 128, transpose_w=True, tag="spconv_fwd")
        assert torch.equal(y[:n, :128], lo[:n]) and torch.equal(y[:n, 128:], hi[:n])
    nd = nv.count_tensor(n_full, cuda)
    first = nv.spconv_fwd(x, koi, nbr, nd, n_full, C, transpose_w=True, tag="spconv_fwd")
    side = torch.cuda.Stream()
    hog_a = torch.empty(256 << 20, dtype=torch.uint8, device=cuda)
    hog_b = torch.empty_like(hog_a)
    stop = torch.cuda.Event()
    with torch.cuda.stream(side):
        for _ in range(60):
            hog_b.copy_(hog_a, non_blocking=True)
        stop.record()
    for i in range(24):
        again = nv.spconv_fwd(x, koi, nbr, nd, n_full, C, transpose_w=True, tag="spconv_fwd")
        assert torch.equal(again, first), i
    stop.synchronize()
    # the weight gradient on the same schedule (k_igemm_wgrad_glds8_256) against the 128-tile kernel (dout cut into two 128-channel
    # halves), full and ragged row counts: the row split of the two plans differs, so f32 sums agree to rounding only - a single stale
    # 64-row tile of the 3000 would be ~3e-4 of the scale
    dy = (torch.randn(n_full, C, device=cuda) * 0.5).bfloat16()
    dys = [dy[:, :128].contiguous(), dy[:, 128:].contiguous()]
    for n in (n_full, n_full - 4321):
        nd = nv.count_tensor(n, cuda)
        dw = nv.spconv_wgrad(x, dy, nbr, nd, 27)
        ref = torch.cat([nv.spconv_wgrad(x, d, nbr, nd, 27) for d in dys], dim=2)
        assert (dw - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()
        assert torch.equal(nv.spconv_wgrad(x, dy, nbr, nd, 27), dw)


@pytest.mark.parametrize("cin,ks", [(64, (1, 1, 1)), (64, (3, 3, 3)), (128, (1, 3, 3)), (192, (3, 1, 1)), (256, (1, 1, 3))])
def test_eight_phase_kernel_short_and_odd_reductions(cuda, cin, ks):
    """The eight-phase kernel's prologue / tail on short reductions (1, 2, 3, 27 ... k-tiles: odd and even counts, a single one), forward
    and transposed (reversed-table) use, ragged row count: bit-identical to the 128-tile kernel on every element."""
    from uni3detr_amd.plugin import dense as dn
    torch.manual_seed(cin + sum(ks))
    B, dims, C = 8, (6, 30, 28), 256                       # 40 320 rows: 158 row tiles of 256 -> the 256 x 256 kernel is dispatched
    pad = tuple(k // 2 for k in ks)
    geom, _ = dn.Lattice.conv(cuda, B, dims, ks, (1, 1, 1), pad)
    n_full = B * dims[0] * dims[1] * dims[2]
    kv = ks[0] * ks[1] * ks[2]
    x = (torch.randn(n_full, cin, device=cuda) * 0.5).bfloat16()
    w = (torch.randn(kv, C, cin, device=cuda) * 0.05).bfloat16()          # n-major [K][Cout][Cin]
    halves = [w[:, :128].contiguous(), w[:, 128:].contiguous()]
    ident = torch.arange(n_full, device=cuda, dtype=torch.int32).view(1, n_full)      # 1x1x1: an explicit table (None = the table-less kernel)
    tables = (ident, ident) if kv == 1 else (geom.nbr_fwd, geom.nbr_bwd)
    for nbr in tables:
        for n in (n_full, n_full - 777):
            nd = nv.count_tensor(n, cuda)
            y = nv.spconv_fwd(x, w, nbr, nd, n_full, C, transpose_w=True, tag="spconv_fwd")
            lo = nv.spconv_fwd(x, halves[0], nbr, nd, n_full, 128, transpose_w=True, tag="spconv_fwd")
            hi = nv.spconv_fwd(x, halves[1], nbr, nd, n_full, 128, transpose_w=True, tag="spconv_fwd")
            assert torch.equal(y[:n, :128], lo[:n]) and torch.equal(y[:n, 128:], hi[:n])
    # and against f32 on a sample of rows (both kernels could share a mistake)
    nbr = tables[0]
    nbt = nbr.t if isinstance(nbr, nv.RevNbr) else nbr
    rows = torch.cat([torch.arange(0, 200, device=cuda), torch.arange(n_full - 200, n_full, device=cuda)])
    y = nv.spconv_fwd(x, w, nbr, nv.count_tensor(n_full, cuda), n_full, C, transpose_w=True, tag="spconv_fwd")
    xf = torch.cat([x.float(), torch.zeros(1, cin, device=cuda)])
    exp = torch.zeros(rows.numel(), C, device=cuda)
    for k in range(kv):
        idx = nbt[k, rows].long()
        idx = torch.where(idx < 0, torch.full_like(idx, n_full), idx)
        exp += xf[idx] @ w[k].float().t()
    assert (y[rows].float() - exp).abs().max().item() <= 1.5e-2 * max(1e-3, exp.abs().max().item())


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_second3d_branch_input_gradients_summed_by_the_convs(cuda, precision):
    """SECOND3D (is_cascade=False): the three branches' input gradients are summed by the first convs' backward launches
    (sp.FanoutToken + addend epilogue, 256 x 256 eight-phase kernel included) - same gradients as autograd's own sums."""
    from uni3detr_amd.plugin import dense as dn
    torch.manual_seed(2)
    B, C = 8, 256
    net = dn.SECOND3D(in_channels=[C, C, C], out_channels=[128, 256, 256], layer_nums=[1, 1, 1], layer_strides=[1, 2, 4], is_cascade=False,
                      conv_cfg=dict(type="Conv3d", kernel=(1, 3, 3), bias=False)).to(cuda).train()
    dt = torch.bfloat16 if precision == "bf16" else torch.float32
    x0 = (torch.randn(B, 15, 40, 40, C, device=cuda) * 0.5).to(dt).permute(0, 4, 1, 2, 3)      # channels_last_3d volume
    res = {}
    for fused in (True, False):
        dn.FANOUT_FUSION = fused
        try:
            for p_ in net.parameters():
                p_.grad = None
            x = x0.clone().requires_grad_(True)
            outs = net(x)
            torch.manual_seed(5)
            loss = sum((o.float() * torch.randn_like(o.float())).sum() for o in outs)
            loss.backward()
            res[fused] = (x.grad.float().clone(), [p_.grad.clone() for p_ in net.parameters()])
        finally:
            dn.FANOUT_FUSION = True
    a, b = res[True], res[False]
    tol = 2e-2 if precision == "bf16" else 1e-5
    assert (a[0] - b[0]).abs().max().item() <= tol * b[0].abs().max().item()
    for u, v in zip(a[1], b[1]):
        assert (u - v).abs().max().item() <= tol * max(1e-6, v.abs().max().item())


@pytest.mark.parametrize("cin,ks,n_cut", [(512, (1, 3, 3), 0), (512, (1, 3, 3), 333), (256, (3, 3, 3), 0), (384, (1, 3, 3), 77)])
def test_eight_phase_256x128_kernel_bit_identical_to_the_128_tile_kernel(cuda, cin, ks, n_cut):
    """k_igemm_glds8_256x128 (three stage buffers, two groups of four waves one barrier apart; dispatched on long reductions with 128-wide
    column tiles: the 12 000-row 512-channel layers) against the 128 x 128-tile kernel, which still serves each 128-column slice on its
    own (too few workgroups for the dispatch rule): bit-identical, ragged row count, forward and reversed tables, odd k-tile counts;
    plus the addend epilogue and 16 launches under HBM load."""
    from uni3detr_amd.plugin import dense as dn
    torch.manual_seed(cin + ks[0])
    B, dims, C = 8, (15, 10, 10), 512
    pad = tuple(k // 2 for k in ks)
    geom, _ = dn.Lattice.conv(cuda, B, dims, ks, (1, 1, 1), pad)
    n_full = B * dims[0] * dims[1] * dims[2]
    kv = ks[0] * ks[1] * ks[2]
    x = (torch.randn(n_full, cin, device=cuda) * 0.5).bfloat16()
    w = (torch.randn(kv, C, cin, device=cuda) * 0.05).bfloat16()
    n = n_full - n_cut
    nd = nv.count_tensor(n, cuda)
    for nbr in (geom.nbr_fwd, geom.nbr_bwd):
        y = nv.spconv_fwd(x, w, nbr, nd, n_full, C, transpose_w=True, tag="spconv_fwd")
        for q in range(4):
            ref = nv.spconv_fwd(x, w[:, q * 128:(q + 1) * 128].contiguous(), nbr, nd, n_full, 128, transpose_w=True, tag="spconv_fwd")
            assert torch.equal(y[:n, q * 128:(q + 1) * 128], ref[:n]), q
    add = torch.randn(n_full, C, device=cuda).bfloat16()
    ya = nv.spconv_fwd(x, w, geom.nbr_fwd, nd, n_full, C, transpose_w=True, addend=add)
    yp = nv.spconv_fwd(x, w, geom.nbr_fwd, nd, n_full, C, transpose_w=True)
    assert ((yp.float() + add.float())[:n] - ya.float()[:n]).abs().max().item() <= 1.6e-2 * ya.float()[:n].abs().max().item()
    side = torch.cuda.Stream()
    hog_a = torch.empty(256 << 20, dtype=torch.uint8, device=cuda)
    hog_b = torch.empty_like(hog_a)
    with torch.cuda.stream(side):
        for _ in range(30):
            hog_b.copy_(hog_a, non_blocking=True)
    for i in range(16):
        assert torch.equal(nv.spconv_fwd(x, w, geom.nbr_fwd, nd, n_full, C, transpose_w=True, tag="spconv_fwd")[:n], yp[:n]), i
    torch.cuda.synchronize()


@pytest.mark.parametrize("seed,n_pts,dims,cut", [(5, 9000, (16, 40, 36), 0), (11, 60000, (12, 64, 64), 777), (3, 300, (8, 8, 8), 0)])
def test_subm_halo_kernel_matches_the_table_kernels(cuda, seed, n_pts, dims, cut):
    """subm_halo.hip (64 -> 64 SubM convs out of each tile's staged DISTINCT rows): the slot tables reproduce the neighbour table
    exactly (integer work: bit-exact), and forward / statistics / input gradient with addend equal the f32 gather-matmul to bf16
    rounding, with a device-side row count below the capacity (dead rows hold NaN), a dense level whose tiles exceed the staged-slot
    budget (global-memory fall-back rows) and a level smaller than one tile."""
    import torch
    from uni3detr_amd import native as nv
    lvl, nbr = _level(seed=seed, n_pts=n_pts, dims=dims)
    n_cap = lvl.n
    n = n_cap - cut
    cnt = nv.count_tensor(n, "cuda") if cut else lvl.n_dev
    nb = nbr.clone()
    if cut:
        nb[:, :n][nb[:, :n] >= n] = -1
    halo = nv.SubmHalo(nb, cnt, n_cap)
    # 1. integer work: tile_rows[tile][loc] == the table, slots sorted and distinct
    T = halo.tiles
    rows = halo.tile_rows.view(T, -1).long()
    loc = (halo.loc.view(T, 27, 16, 8).long() & 0xffff).permute(0, 1, 3, 2).reshape(T, 27, 128)         # [tile][k][mt * 16 + r16]
    tc = halo.tile_cnt.long()
    assert int(tc.max()) <= 27 * 128 + 1 and int(loc.max()) < int(tc.max())
    recon = torch.gather(rows, 1, loc.reshape(T, -1)).view(T, 27, 128).permute(1, 0, 2).reshape(27, -1)[:, :n]
    assert torch.equal(recon.int(), nb[:, :n])
    for t in (0, T // 2, T - 1):
        r = rows[t, 1:int(tc[t])]
        assert (r[1:] > r[:-1]).all()
    # 2. forward + statistics, input gradient with addend
    torch.manual_seed(seed)
    x = torch.randn(n_cap, 64, device="cuda").bfloat16()
    add = torch.randn(n_cap, 64, device="cuda").bfloat16()
    if cut:
        x[n:] = float("nan"); add[n:] = float("nan")
    w = (torch.randn(27, 64, 64, device="cuda") * 0.1).bfloat16()               # n-major [K][out][reduction]
    wp = nv.subm_halo_wpack(w)
    y, stats, tr = nv.subm_halo_conv(x, wp, halo, want_stats=True)
    exp = _ref_conv(x[:n], w.transpose(1, 2), nb, n)
    sc = exp.abs().max()
    assert torch.isfinite(y[:n]).all() and (y[:n].float() - exp).abs().max() / sc < 6e-3
    assert tr == 128 and stats.shape == (T, 2, 64)
    yf = y[:n].double()
    assert (stats[:, 0].sum(0) - yf.sum(0)).abs().max() < 1e-3 * yf.abs().sum(0).max()
    assert (stats[:, 1].sum(0) - (yf * yf).sum(0)).abs().max() < 1e-4 * (yf * yf).sum(0).max()
    assert torch.equal(nv.subm_halo_conv(x, wp, halo)[:n], y[:n])                 # deterministic, statistics do not change the output
    # rows beyond the staged slots are read from global memory (test hook: stage only 150 / 40 slots): same products, same order
    assert int(halo.tile_cnt.max()) > 40
    for ms in (150, 40):
        assert torch.equal(nv.subm_halo_conv(x, wp, halo, max_slots=ms)[:n], y[:n]), ms
    # offsets reversed == the transposed table (test_subm_transposed_table_is_the_reversed_forward_table)
    g = nv.subm_halo_conv(x, wp, halo, krev=True, addend=add)
    expg = _ref_conv(x[:n], w.transpose(1, 2), nb.flip(0), n) + add[:n].float()
    assert (g[:n].float() - expg).abs().max() / expg.abs().max() < 6e-3
    # against the LDS-DMA kernels on the same operands: same products, different f32 summation order -> one bf16 ulp at most
    ref = nv.spconv_fwd(x, w, nb, cnt, n_cap, 64, transpose_w=True)[:n].float()
    assert (y[:n].float() - ref).abs().max() / sc < 8e-3


def test_subm_halo_used_by_the_64_channel_blocks(cuda):
    """sparse._SparseConv routes 64 -> 64 SubM convs (forward, statistics epilogue, input gradient with the residual addend) through
    the halo kernel; result and gradients equal the table path's to bf16 rounding."""
    import torch
    from uni3detr_amd import native as nv, sparse as sp
    lvl, _ = _level(seed=7, n_pts=30000, dims=(12, 48, 48))
    torch.manual_seed(1)
    x0 = torch.randn(lvl.n, 64, device="cuda").bfloat16()
    w0 = (torch.randn(3, 3, 3, 64, 64, device="cuda") * 0.05)
    dy = torch.randn(lvl.n, 64, device="cuda").bfloat16()
    res = {}
    for on in (True, False):
        sp.SUBM_HALO = on
        try:
            lv = sp.Level(lvl.grid, lvl.coords, lvl.n, lvl.n_dev)
            x = x0.clone().requires_grad_(True)
            w = w0.clone().requires_grad_(True)
            y, st = sp._SparseConv.apply(x, w, sp.subm_geom(lv), "dhwio", True)
            assert (lv._halo is not None) == on
            y.backward(dy)
            res[on] = (y.detach().float(), st.double().sum(0), x.grad.float(), w.grad.float())
        finally:
            sp.SUBM_HALO = True
    for a, b, tol in zip(res[True], res[False], (8e-3, 1e-3, 8e-3, 1e-5)):
        assert (a - b).abs().max() / b.abs().max() < tol


@pytest.mark.parametrize("seed,n_pts,dims,cut", [(5, 9000, (16, 40, 36), 0), (11, 60000, (12, 64, 64), 777), (3, 300, (8, 8, 8), 0)])
def test_subm_halo_weight_gradient(cuda, seed, n_pts, dims, cut):
    """k_subm_halo_wgrad64 (both MFMA operands by transpose reads out of the tile's staged distinct rows / dy tile, offsets split
    over four groups of persistent workgroups): every offset's dW against an f32 gather-matmul; a device-side row count below the
    capacity with NaN in the dead rows; a dense level whose tiles exceed the stage buffer (the per-offset gather fall-back - checked
    to be the case); a level smaller than one tile; zero rows; bitwise repeatable."""
    import torch
    from uni3detr_amd import native as nv
    lvl, nbr = _level(seed=seed, n_pts=n_pts, dims=dims)
    n_cap = lvl.n
    n = n_cap - cut
    cnt = nv.count_tensor(n, "cuda") if cut else lvl.n_dev
    nb = nbr.clone()
    if cut:
        nb[:, :n][nb[:, :n] >= n] = -1
    halo = nv.SubmHalo(nb, cnt, n_cap)
    slots = 150 if cut else 0                                                     # test hook: tiles with more distinct rows take the fall-back path
    assert not cut or int(halo.tile_cnt.max()) > slots
    torch.manual_seed(seed)
    x = torch.randn(n_cap, 64, device="cuda").bfloat16()
    dy = torch.randn(n_cap, 64, device="cuda").bfloat16()
    if cut:
        x[n:] = float("nan"); dy[n:] = float("nan")
    got = nv.subm_halo_wgrad(x, dy, halo, max_slots=slots)
    xf = torch.cat([x[:n].float(), torch.zeros(1, 64, device="cuda")])
    exp = torch.stack([xf[torch.where(nb[k, :n] < 0, torch.full_like(nb[k, :n], n), nb[k, :n]).long()].t() @ dy[:n].float() for k in range(27)])
    assert torch.isfinite(got).all()
    assert (got - exp).abs().max() / exp.abs().max() < 2e-5                       # bf16 products are exact in f32; only the summation order differs
    ref = nv.spconv_wgrad(x, dy, nb, cnt, 27)
    assert (got - ref).abs().max() / exp.abs().max() < 2e-5
    assert torch.equal(nv.subm_halo_wgrad(x, dy, halo, max_slots=slots), got)      # deterministic
    assert (nv.subm_halo_wgrad(x, dy, halo) - got).abs().max() / exp.abs().max() < 2e-5      # staged path == fall-back path
    out = torch.empty(27 * 4096, device="cuda")
    assert nv.subm_halo_wgrad(x, dy, halo, out=out, max_slots=slots).data_ptr() == out.data_ptr() and torch.equal(out.view(27, 64, 64), got)
    zero = nv.SubmHalo(nb, nv.count_tensor(0, "cuda"), n_cap)
    assert (nv.subm_halo_wgrad(x, dy, zero) == 0).all()


@pytest.mark.parametrize("seed,n_pts,dims,cut", [(5, 9000, (16, 40, 36), 0), (11, 60000, (12, 64, 64), 777)])
def test_subm_halo_128_channel_kernel(cuda, seed, n_pts, dims, cut):
    """k_subm_halo128 (128 -> 128 SubM convs: waves split the output columns, the 256-byte rows staged one 64-channel half at a time):
    forward + per-tile statistics, input gradient (offsets reversed) with addend, the global-memory fall-back for rows past the staged
    slots (max_slots hook), a device-side row count below the capacity with NaN in the dead rows; against the f32 gather-matmul and the
    LDS-DMA tiled kernel."""
    import torch
    from uni3detr_amd import native as nv
    lvl, nbr = _level(seed=seed, n_pts=n_pts, dims=dims)
    n_cap = lvl.n
    n = n_cap - cut
    cnt = nv.count_tensor(n, "cuda") if cut else lvl.n_dev
    nb = nbr.clone()
    if cut:
        nb[:, :n][nb[:, :n] >= n] = -1
    halo = nv.SubmHalo(nb, cnt, n_cap)
    torch.manual_seed(seed)
    x = torch.randn(n_cap, 128, device="cuda").bfloat16()
    add = torch.randn(n_cap, 128, device="cuda").bfloat16()
    if cut:
        x[n:] = float("nan"); add[n:] = float("nan")
    w = (torch.randn(27, 128, 128, device="cuda") * 0.07).bfloat16()             # n-major [K][out][reduction]
    wp = nv.subm_halo_wpack(w)
    y, stats, tr = nv.subm_halo_conv(x, wp, halo, want_stats=True)
    exp = _ref_conv(x[:n], w.transpose(1, 2), nb, n)
    sc = exp.abs().max()
    assert torch.isfinite(y[:n]).all() and (y[:n].float() - exp).abs().max() / sc < 6e-3
    assert tr == 128 and stats.shape == (halo.tiles, 2, 128)
    yf = y[:n].double()
    assert (stats[:, 0].sum(0) - yf.sum(0)).abs().max() < 1e-3 * yf.abs().sum(0).max()
    assert (stats[:, 1].sum(0) - (yf * yf).sum(0)).abs().max() < 1e-4 * (yf * yf).sum(0).max()
    assert torch.equal(nv.subm_halo_conv(x, wp, halo)[:n], y[:n])
    for ms in (150, 40):
        assert torch.equal(nv.subm_halo_conv(x, wp, halo, max_slots=ms)[:n], y[:n]), ms
    g = nv.subm_halo_conv(x, wp, halo, krev=True, addend=add)
    expg = _ref_conv(x[:n], w.transpose(1, 2), nb.flip(0), n) + add[:n].float()
    assert (g[:n].float() - expg).abs().max() / expg.abs().max() < 6e-3
    ref = nv.spconv_fwd(x, w, nb, cnt, n_cap, 128, transpose_w=True)[:n].float()
    assert (y[:n].float() - ref).abs().max() / sc < 8e-3


# ---------------------------------------------------------------------------------------------------------------------------
# split-bf16 convolutions (`mixed` precision: the reference keeps SparseEncoderHD + SECOND3D in fp32, sparse_encoder_hd.py:62-64):
# f32 rows in and out, three bf16 MFMA products per product on the LDS-DMA kernels (u3d_igemm_fwd_split_bf16, sparse.split_scope)
# ---------------------------------------------------------------------------------------------------------------------------
def test_split_rows_is_an_exact_two_term_expansion(cuda):
    torch.manual_seed(1)
    x = (torch.randn(1000, 64, device=cuda) * torch.logspace(-6, 6, 64, device=cuda)).contiguous()
    n_dev = torch.tensor([777], dtype=torch.int32, device=cuda)
    p = nv.split_rows(x, n_dev)
    hi, lo = p[:777].float(), p[1000:1777].float()
    assert torch.equal(p[:777], x[:777].to(torch.bfloat16))
    assert torch.equal(p[1000:1777], (x[:777] - hi).to(torch.bfloat16))
    rel = ((hi + lo) - x[:777]).abs() / x[:777].abs().clamp_min(1e-30)
    assert float(rel.max()) <= 2.0 ** -16          # two bf16 terms carry 16 mantissa bits


@pytest.mark.parametrize("cin,cout,kvol,wide_rows", [(64, 64, 27, False), (64, 128, 27, False), (128, 128, 27, False), (128, 256, 1, False),
                                                     (256, 256, 27, True), (16, 16, 27, False), (16, 32, 27, False), (32, 32, 27, False),
                                                     (32, 64, 27, False), (64, 32, 27, False)])
def test_split_bf16_conv_forward_backward_match_f32_oracle(cuda, cin, cout, kvol, wide_rows):
    """_SparseConv inside sparse.split_scope(): forward, input gradient and weight gradient against oracle/geometry.py's f32 conv at
    5e-5 of the result's scale (bf16 kernels on bf16-rounded operands sit at 1e-2: this is f32-grade), incl. the fused BatchNorm
    statistics of the f32 output; wide_rows: enough rows for the 256 x 256 eight-phase kernel's f32-output instantiation."""
    from uni3detr_amd import sparse as sp
    torch.manual_seed(cin + cout + kvol)
    B = 3 if wide_rows else 2
    rc = _level0(cuda, B, 18000 if wide_rows else 2500)          # 3 x 16 000 voxels: 188 row tiles of 256
    dims = (128, 320, 320)
    coors = torch.from_numpy(rc).to(cuda)
    lvl, rank = sp.level_from_coors(coors, B, dims)
    n = lvl.n
    if kvol == 27:
        geom = sp.subm_geom(lvl)
        ref_nbr = geom.nbr_fwd.cpu().numpy()[:, :n].astype(np.int64)
        wshape = (3, 3, 3, cin, cout)
    else:
        geom = sp.ConvGeom(None, None, n, lvl.n_dev, n, lvl.n_dev)
        ref_nbr = np.arange(n, dtype=np.int64)[None]
        wshape = (1, 1, 1, cin, cout)
    x = torch.randn(n, cin)
    w = torch.randn(*wshape) * (1.0 / np.sqrt(cin * min(kvol, 9)))
    gy = torch.randn(n, cout)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yr = og.sparse_conv(xr, wr.view(kvol, cin, cout), ref_nbr)
    yr.backward(gy)
    xd, wd = x.to(cuda).requires_grad_(True), torch.nn.Parameter(w.to(cuda))
    with sp.split_scope(True):
        y, stats = sp._SparseConv.apply(xd, wd, geom, "dhwio", True, None, None)
    narrow = cin % 64 != 0 or cout % 64 != 0                         # the direct-operand kernels: three accumulating launches, no statistics
    assert y.dtype == torch.float32 and (stats.numel() > 0) == (not narrow)
    calls = []
    real = nv.spconv_fwd
    nv.spconv_fwd = lambda *a, **k: (calls.append(1), real(*a, **k))[1]          # the exact-f32 kernels must not be what served the backward
    try:
        y.backward(gy.to(cuda))
    finally:
        nv.spconv_fwd = real
    assert not calls
    tol = 5e-5
    assert (y.detach().cpu() - yr.detach()).abs().max().item() <= tol * yr.abs().max().item()
    assert (xd.grad.cpu() - xr.grad).abs().max().item() <= tol * xr.grad.abs().max().item()
    assert (wd.grad.cpu() - wr.grad).abs().max().item() <= tol * wr.grad.abs().max().item()
    if narrow:
        return
    tr = stats._u3d_tile_rows
    s = stats.sum(0).cpu()
    np.testing.assert_allclose(s[0].numpy(), y.detach().double().sum(0).cpu().numpy(), rtol=1e-5, atol=1e-4 * float(y.abs().max()) * n ** 0.5)
    np.testing.assert_allclose(s[1].numpy(), (y.detach().double() ** 2).sum(0).cpu().numpy(), rtol=1e-5)
    assert stats.shape[0] == (n + tr - 1) // tr


@pytest.mark.parametrize("c,res,rowmap", [(16, False, False), (64, True, False), (256, False, True), (512, False, False), (128, False, False)])
def test_bn_passes_write_the_planes_a_split_product_reads(cuda, c, res, rowmap):
    """u3d_bn_apply / u3d_bn_bwd_apply with planes (round 6): the BatchNorm apply pass of the fp32 modules also leaves its output as the
    hi / lo bf16 planes of a split-bf16 product, the backward pass the planes of dx - bit for bit what u3d_split_rows_f32 of the same
    tensor holds (padding rows of a capacity-sized tensor: zeros), and y / dx themselves unchanged."""
    torch.manual_seed(c)
    n_cap, n = 3000, 2777
    x = (torch.randn(n_cap, c, device=cuda) * 2 + 0.5).contiguous()
    x[n:] = float("nan")                                   # capacity padding holds garbage
    r = torch.randn(n_cap, c, device=cuda) if res else None
    gamma, beta = torch.rand(c, device=cuda) + 0.5, torch.randn(c, device=cuda) * 0.1
    nd = torch.tensor([n], dtype=torch.int32, device=cuda)
    mean, invstd = nv.bn_forward_stats(x, nd, 1e-3, 0.1)
    rm = None
    if rowmap:
        perm = torch.randperm(n, device=cuda)
        rm = torch.cat([perm, torch.arange(n, n_cap, device=cuda)]).int()
    y0 = nv.bn_apply(x, mean, invstd, gamma, beta, r, True, nd, rm)
    y1, pl = nv.bn_apply(x, mean, invstd, gamma, beta, r, True, nd, rm, want_planes=True)
    assert pl is not None and pl.shape == (2 * n_cap, c) and pl.dtype == torch.bfloat16
    live = rm[:n].long() if rowmap else torch.arange(n, device=cuda)
    assert torch.equal(y0[live], y1[live])
    y1c = y1.clone()
    y1c[n:] = 0                                            # rows past the count: unwritten in y, zero in the planes
    ref = nv.split_rows(y1c, nd)
    assert torch.equal(pl, ref)
    assert not bool(torch.isnan(pl.float()).any())
    # backward
    dy = torch.randn(n_cap, c, device=cuda)
    sums = nv.bn_bwd_stats(dy, None if not res else y1, x, mean, invstd, True, nd, gamma, beta, rm)
    dx0, dres0 = nv.bn_bwd_apply(dy, None if not res else y1, x, mean, invstd, gamma, sums, True, nd, res, beta, rm)
    dx1, dres1, dpl = nv.bn_bwd_apply(dy, None if not res else y1, x, mean, invstd, gamma, sums, True, nd, res, beta, rm, want_planes=True)
    assert dpl is not None and torch.equal(dx0[:n], dx1[:n]) and (not res or torch.equal(dres0[:n], dres1[:n]))
    d = dx1.clone()
    d[n:] = 0
    assert torch.equal(dpl, nv.split_rows(d, nd))


@pytest.mark.parametrize("c", [24, 64])
def test_bn_planes_retry_where_the_fused_pass_does_not_take_the_shape(cuda, c):
    """want_planes on f32 rows, one row past a 256-row block and with a device count below the capacity: c = 64 runs the fused pass,
    c = 24 (a multiple of 4, but 256 % (24 / 4) != 0) is answered U3D_ERR_UNSUPPORTED and retried without planes -> (y, None) /
    (dx, dres, None).  y / dx are the bits of the call without want_planes either way."""
    torch.manual_seed(c)
    n, live = 257, 200
    x = (torch.randn(n, c, device=cuda) * 2 + 0.5).contiguous()
    x[live:] = float("nan")
    r = torch.randn(n, c, device=cuda)
    gamma, beta = torch.rand(c, device=cuda) + 0.5, torch.randn(c, device=cuda) * 0.1
    nd = torch.tensor([live], dtype=torch.int32, device=cuda)
    mean, invstd = nv.bn_forward_stats(x, nd, 1e-3, 0.1)
    bits = lambda t: t[:live].view(torch.int32)      # noqa: E731
    y0 = nv.bn_apply(x, mean, invstd, gamma, beta, r, True, nd)
    y1, pl = nv.bn_apply(x, mean, invstd, gamma, beta, r, True, nd, want_planes=True)
    assert bool(torch.isfinite(y0[:live]).all()) and torch.equal(bits(y0), bits(y1))
    dy = torch.randn(n, c, device=cuda)
    sums = nv.bn_bwd_stats(dy, y0, x, mean, invstd, True, nd, gamma, beta)
    dx0, dres0 = nv.bn_bwd_apply(dy, y0, x, mean, invstd, gamma, sums, True, nd, True, beta)
    dx1, dres1, dpl = nv.bn_bwd_apply(dy, y0, x, mean, invstd, gamma, sums, True, nd, True, beta, want_planes=True)
    assert bool(torch.isfinite(dx0[:live]).all()) and torch.equal(bits(dx0), bits(dx1)) and torch.equal(bits(dres0), bits(dres1))
    if c == 24:
        assert pl is None and dpl is None
        return
    for planes, t in ((pl, y1), (dpl, dx1)):
        assert planes.shape == (2 * n, c) and planes.dtype == torch.bfloat16
        ref = nv.split_rows(t, nd).view(2, n, c)
        assert torch.equal(planes.view(2, n, c)[:, :live].view(torch.int16), ref[:, :live].view(torch.int16))
        assert not bool(planes.view(2, n, c)[:, live:].view(torch.int16).any())      # rows past the count: zeros in both planes


def test_split_convs_pick_up_the_planes_their_batchnorm_wrote(cuda):
    """A conv -> BN -> ReLU -> conv -> BN chain inside split_scope: with sparse.BN_PLANES the second convolution's input planes and the first
    convolution's output-gradient planes come from the BatchNorm passes - same bits as with separate u3d_split_rows_f32 launches, and
    the separate launches are gone (counted through native.split_rows)."""
    import torch.nn as nn
    from uni3detr_amd import sparse as sp
    from uni3detr_amd.plugin import dense as D
    torch.manual_seed(3)
    B, dims, C = 2, (3, 12, 12), 64
    convs = [nn.Conv3d(C, C, (1, 3, 3), padding=(0, 1, 1), bias=False).to(cuda) for _ in range(2)]
    bns = [nn.BatchNorm3d(C, eps=1e-3, momentum=0.01).to(cuda).train() for _ in range(2)]
    x0 = torch.randn(B, C, *dims, device=cuda).clamp_min(0).contiguous(memory_format=torch.channels_last_3d)
    res, calls = {}, {}
    orig = nv.split_rows
    for on in (True, False):
        sp.BN_PLANES = on
        cnt = [0]

        def counting(*a, **k):
            cnt[0] += 1
            return orig(*a, **k)
        nv.split_rows = counting
        try:
            x = x0.clone().requires_grad_(True)
            for m in convs + bns:
                m.zero_grad(set_to_none=True)
            with sp.split_scope(True):
                rows, Bb, dd = D.to_rows(x)
                for cv, bn in zip(convs, bns):
                    rows, dd = D.conv_bn_relu(rows, Bb, dd, cv, bn)
                y = D.to_volume(rows, Bb, dd)
            (y * y).sum().backward()
            torch.cuda.synchronize()
        finally:
            nv.split_rows = orig
            sp.BN_PLANES = True
        res[on] = (y.detach().clone(), x.grad.clone(), [c.weight.grad.clone() for c in convs])
        calls[on] = cnt[0]
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
    assert all(torch.equal(a, b) for a, b in zip(res[True][2], res[False][2]))
    # separate passes: 2 inputs + 2 output gradients; with the planes from the BatchNorm passes only the very first input is split on its own
    assert calls[False] == 4 and calls[True] == 1, calls


def test_weight_splits_of_a_step_in_one_launch(cuda):
    """native.Split3Set (u3d_split3_weights_batch): the (hi, lo, hi) bf16 planes of every convolution weight a split scope asks for are
    refreshed by ONE launch at the top of the next scope - bit-identical to the per-request launches, recomputed after the parameters
    change (in-place torch update: version check; raw-pointer update + refresh: TrainStep's flat AdamW), entries of dead parameters pruned."""
    import gc
    import torch.nn as nn
    from uni3detr_amd import sparse as sp
    torch.manual_seed(5)
    ws = [nn.Parameter(torch.randn(3, 3, 3, 16, 32, device=cuda)), nn.Parameter(torch.randn(64, 128, 1, 3, 3, device=cuda)),
          nn.Parameter(torch.randn(1, 1, 1, 128, 256, device=cuda))]
    lay = ["dhwio", "oidhw", "dhwio"]
    ref = lambda w, l, nm: (nv.SPLIT3_BATCH, setattr(nv, "SPLIT3_BATCH", False), nv.split3_weights(w, l, nm), setattr(nv, "SPLIT3_BATCH", True))[2]      # noqa: E731
    own = nv.Split3Set()
    with sp.split_scope(True, own):                                    # first scope: per-request launches, the set fills up
        first = [(nv.split3_weights(w, l, True), nv.split3_weights(w, l, False)) for w, l in zip(ws, lay)]
    assert len(own.entries) == 6 and not own.fresh
    calls = [0]
    orig = nv.lib().u3d_split3_weights
    with sp.split_scope(True, own):                                    # second scope: one batched launch, every request served from it
        assert own.fresh and own.njobs == 6
        got = [(nv.split3_weights(w, l, True), nv.split3_weights(w, l, False)) for w, l in zip(ws, lay)]
        for (a, b), (fa, fb) in zip(got, first):
            assert a.data_ptr() == fa.data_ptr() and b.data_ptr() == fb.data_ptr()          # the cached buffers
    for (a, b), w, l in zip(got, ws, lay):
        assert torch.equal(a, ref(w, l, True)) and torch.equal(b, ref(w, l, False))
    # parameters change: (1) in-place torch update inside a scope -> the version check refuses the cached planes
    with sp.split_scope(True, own):
        with torch.no_grad():
            ws[0].mul_(1.5)
        a = nv.split3_weights(ws[0], lay[0], True)
        assert torch.equal(a, ref(ws[0], lay[0], True))
    # (2) a raw update (no version bump) followed by the next scope's refresh
    with torch.no_grad():
        ws[1].data.view(-1)[:1000] += 1.0
    with sp.split_scope(True, own):
        assert torch.equal(nv.split3_weights(ws[1], lay[1], False), ref(ws[1], lay[1], False))
    # (3) a parameter dies: its jobs leave the table at the next refresh (nothing reads freed memory)
    del ws[2], got, first, a, w, l
    gc.collect()
    with sp.split_scope(True, own):
        assert len(own.entries) == 4 and own.njobs == 4
    torch.cuda.synchronize()


def test_batched_row_split_and_three_way_sum(cuda):
    """u3d_split_rows_batch (several strided f32 row matrices -> hi / lo planes in one launch; > 32 jobs = several launches) against
    u3d_split_rows_f32 on contiguous copies; u3d_sum3_f32 against (a + b) + c."""
    torch.manual_seed(2)
    big = torch.randn(700, 1024, device=cuda) * torch.logspace(-4, 4, 1024, device=cuda)
    views = [big[:, o:o + w] for o, w in ((0, 256), (256, 512), (768, 4), (772, 12), (784, 240))] + [torch.randn(33, 64, device=cuda)]
    views = views * 7                                       # 42 jobs: two launches
    got = nv.split_rows_batch(views)
    for v, g in zip(views, got):
        nd = torch.tensor([v.shape[0]], dtype=torch.int32, device=cuda)
        assert torch.equal(g, nv.split_rows(v.contiguous(), nd))
    a, b, c = (torch.randn(27, 64, 128, device=cuda) for _ in range(3))
    assert torch.equal(nv.sum3(a, b, c), (a + b) + c)
    two = torch.randn(54, 64, 128, device=cuda)
    assert torch.equal(nv.sum3(two[:27], two[27:], c), (two[:27] + two[27:]) + c)


def test_census_entry_of_every_conv_wrapper(cuda):
    """Each of the nine convolution wrappers of native.py under KernelTimer("census"): ONE census entry per call, under the documented
    tag, whose dict equals the one worked out here from the table and the shapes (SURVEY.md §8d pricing: element size 2 / s, f32 weights
    for a weight gradient, a split product priced as the f32 conv it stands for) - and the same outputs, bit for bit, under
    KernelTimer("time") and with no timer."""
    from uni3detr_amd import sparse as sp
    lvl, nbr = _level(seed=3, n_pts=300, dims=(8, 8, 8))
    n, nd = lvl.n, lvl.n_dev
    halo = nv.SubmHalo(nbr, nd, n)
    assert halo.ok
    rev = nv.RevNbr(nbr)
    torch.manual_seed(1)
    ident = torch.arange(n, dtype=torch.int32, device=cuda).view(1, -1)
    tri = lambda t: torch.cat([t, t, torch.where(t >= 0, t + n, t)], 0).contiguous()      # noqa: E731  (t, t, t + plane)
    xb = {c: torch.randn(n, c, device=cuda).bfloat16() for c in (32, 64, 128)}
    xf = torch.randn(n, 32, device=cuda)
    wb = {(k, c): (torch.randn(k, c, c, device=cuda) * 0.1).bfloat16() for k, c in ((27, 32), (27, 64), (27, 128), (1, 128), (81, 32), (81, 128), (3, 128))}
    wf = torch.randn(27, 32, 32, device=cuda) * 0.1
    pk = {c: nv.subm_halo_wpack(wb[(27, c)]) for c in (64, 128)}
    sh = {c: torch.randn(c, device=cuda) for c in (32, 64, 128)}
    xs = {c: nv.split_rows(torch.randn(n, c, device=cuda), nd) for c in (32, 128)}
    kind = nv.CALL_KIND
    pairs = int((nbr[:, :n] >= 0).sum())
    assert 0 < pairs < 27 * n

    def entry(cin, cout, kvol, p, s=2, w=None, v2=True, split=False):
        w = s if w is None else w
        d = dict(kind=kind, v2=v2, n_in=n, n_out=n, cin=cin, cout=cout, kvol=kvol, pairs=p,
                 bytes=n * cin * s + n * cout * s + 8 * p + kvol * cin * cout * w, flops=2 * p * cin * cout)
        if split:
            d["split"] = True
        return d

    def fwd_stats(w, table):
        r = nv.spconv_fwd(xb[128], w, table, nd, n, 128, transpose_w=True, tag="spconv_fwd", want_stats=True)
        return r if r[1] is not None else None          # None: no statistics came back

    calls = [     # (what runs, tag, census dict)
        (lambda: fwd_stats(wb[(27, 128)], nbr), "spconv_fwd", entry(128, 128, 27, pairs)),
        (lambda: fwd_stats(wb[(1, 128)], None), "spconv_fwd", entry(128, 128, 1, n)),
        (lambda: nv.subm_halo_wgrad(xb[64], xb[64].flip(0).contiguous(), halo), "spconv_wgrad", entry(64, 64, 27, pairs, w=4)),
        (lambda: nv.subm_halo_conv(xb[64], pk[64], halo), "spconv_fwd", entry(64, 64, 27, pairs)),
        (lambda: nv.subm_halo_conv(xb[128], pk[128], halo, krev=True, addend=xb[128], want_stats=True, tag="spconv_dgrad"), "spconv_dgrad",
         entry(128, 128, 27, pairs)),
        (lambda: nv.subm_halo_conv_affine(xb[64], pk[64], halo, sh[64], True), "spconv_fwd", entry(64, 64, 27, pairs)),
        (lambda: nv.subm_halo_conv_affine(xb[128], pk[128], halo, sh[128], False, addend=xb[128]), "spconv_fwd", entry(128, 128, 27, pairs)),
        (lambda: nv.spconv_fwd(xb[32], wb[(27, 32)], nbr, nd, n, 32), "spconv_fwd", entry(32, 32, 27, pairs)),
        (lambda: nv.spconv_fwd(xb[32], wb[(27, 32)], rev, nd, n, 32, transpose_w=True, addend=xb[32]), "spconv_dgrad", entry(32, 32, 27, pairs)),
        (lambda: nv.spconv_fwd(xb[32], wb[(27, 32)], nbr, nd, n, 32, transpose_w=True, tag="spconv_fwd"), "spconv_fwd", entry(32, 32, 27, pairs)),
        (lambda: nv.spconv_fwd(xf, wf, nbr, nd, n, 32), "spconv_fwd", entry(32, 32, 27, pairs, s=4, v2=False)),
        (lambda: nv.spconv_fwd(xf, wf, rev, nd, n, 32, transpose_w=True), "spconv_dgrad", entry(32, 32, 27, pairs, s=4, v2=False)),
        (lambda: nv.spconv_fwd_split_direct(xs[32], wb[(81, 32)], nbr, nd, n, 32), "spconv_fwd", entry(32, 32, 27, pairs, s=4, split=True)),
        (lambda: nv.spconv_fwd_split_direct(xs[32], wb[(81, 32)], rev, nd, n, 32, tag="spconv_dgrad"), "spconv_dgrad",
         entry(32, 32, 27, pairs, s=4, split=True)),
        (lambda: nv.igemm_fwd_affine(xb[128], wb[(27, 128)], nbr, sh[128], True, nd, n), "spconv_fwd", entry(128, 128, 27, pairs)),
        (lambda: nv.igemm_fwd_affine(xb[128], wb[(1, 128)], None, sh[128], False, nd, n), "spconv_fwd", entry(128, 128, 1, n)),
        (lambda: nv.igemm_direct_affine(xb[32], wb[(27, 32)], nbr, sh[32], True, nd, n, addend=xb[32]), "spconv_fwd", entry(32, 32, 27, pairs)),
        (lambda: nv.spconv_fwd_split(xs[128], wb[(81, 128)], tri(nbr), nd, n, 128, want_stats=True), "spconv_fwd",
         entry(128, 128, 27, pairs, s=4, split=True)),
        (lambda: nv.spconv_fwd_split(xs[128], wb[(3, 128)], tri(ident), nd, n, 128, tag="spconv_dgrad"), "spconv_dgrad",
         entry(128, 128, 1, n, s=4, split=True)),
        (lambda: nv.spconv_wgrad(xb[32], xb[32].flip(0).contiguous(), nbr, nd, 27), "spconv_wgrad", entry(32, 32, 27, pairs, w=4)),
        (lambda: nv.spconv_wgrad(xb[128], xb[128].flip(0).contiguous(), None, nd, 1, out_oik=True), "spconv_wgrad", entry(128, 128, 1, n, w=4)),
        (lambda: nv.spconv_wgrad(xf, xf.flip(0).contiguous(), nbr, nd, 27), "spconv_wgrad", entry(32, 32, 27, pairs, s=4, w=4, v2=False)),
    ]

    def run(timer):
        nv.TIMER = timer
        outs = []
        for i, (fn, _, _) in enumerate(calls):
            before = len(timer.calls) if timer is not None else 0
            r = fn()
            assert r is not None, i                      # the wrapper's own kernel served the call
            if timer is not None:
                assert len(timer.calls) == before + 1, i
            outs.append([t for t in (r if isinstance(r, tuple) else (r,)) if torch.is_tensor(t)])
        return outs

    try:
        census, timed = nv.KernelTimer("census"), nv.KernelTimer("time")
        a = run(census)
        assert len(census.census) == len(calls)
        for i, ((tag, meta), (_, want_tag, want)) in enumerate(zip(census.census, calls)):
            assert tag == want_tag and meta == want, (i, tag, meta, want)
        assert [t for t, _, _ in census.calls] == [c[1] for c in calls]
        b = run(timed)
        assert timed.census == [] and [t for t, _, _ in timed.calls] == [c[1] for c in calls]
        c = run(None)
    finally:
        nv.TIMER = None
    for i, (p, q, r) in enumerate(zip(a, b, c)):
        assert len(p) == len(q) == len(r) > 0
        for u, v, w in zip(p, q, r):
            assert torch.equal(u, v) and torch.equal(u, w), i
    # (the calls compute what they say: the first spconv_fwd against the gather-matmul reference)
    exp = _ref_conv(xb[32], wb[(27, 32)], nbr, n)
    assert (a[7][0].float() - exp).abs().max() / exp.abs().max() < 1e-2
    assert all(ms >= 0 for _, ms in timed.durations_ms())


def _grads_with_and_without_tokens(build, x0, params):
    """build(x, params, tokens: bool) -> (output, the tokens it made); -> {tokens: [x.grad, *param grads]} for one fixed output gradient."""
    from uni3detr_amd import sparse as sp
    res = {}
    for tokens in (True, False):
        x = x0.clone().requires_grad_(True)
        ps = [p.clone().requires_grad_(True) for p in params]
        y, toks = build(x, ps, tokens)
        torch.manual_seed(77)
        y.backward(torch.randn(y.shape, device=y.device).to(y.dtype))
        for t in toks:
            if isinstance(t, sp.ResidualToken):
                assert t.dres is None
            else:
                assert t.acc is None and t.remaining == t.n
        res[tokens] = [x.grad.float()] + [p.grad.float() for p in ps]
    return res


GRAD_ADDEND_ROUTES = ["bf16_table", "bf16_halo", "bf16_direct", "f32_exact", "split_wide", "split_narrow", "strided_bf16", "strided_split"]


@pytest.mark.parametrize("route", GRAD_ADDEND_ROUTES)
def test_gradient_addends_same_on_every_route(cuda, route):
    """The residual identity's gradient (sp.ResidualToken) and the other fan-out branches' sum (sp.FanoutToken) enter a conv's input gradient
    on every route - in the kernel's epilogue or added after it - and give what autograd's own sums give: x.grad and the weight gradients
    with the tokens against the same graph with None in their place.  bf16: 1.6e-2 of the result's max (the two-pass form rounds
    twice, as test_input_gradient_with_addend_epilogue); f32 and split-bf16: 1e-5 (as the SECOND3D fan-out test)."""
    from uni3detr_amd import sparse as sp
    if route.startswith("strided"):
        return _strided_route_addends(cuda, route == "strided_bf16")
    c = {"bf16_table": 128, "bf16_halo": 64, "bf16_direct": 32, "f32_exact": 32, "split_wide": 128, "split_narrow": 32}[route]
    bf16 = route.startswith("bf16")
    lvl0, _ = _level() if route == "bf16_halo" else _level(seed=3, n_pts=300, dims=(8, 8, 8))
    assert (lvl0.n >= 4096) == (route == "bf16_halo")
    tol = 1.6e-2 if bf16 else 1e-5
    torch.manual_seed(c)
    x0 = torch.randn(lvl0.n, c, device=cuda).to(torch.bfloat16 if bf16 else torch.float32)
    ws = [torch.randn(3, 3, 3, c, c, device=cuda) * (0.6 / (27 * c) ** 0.5) for _ in range(2)]
    levels = []

    def geom_of():
        lv = sp.Level(lvl0.grid, lvl0.coords, lvl0.n, lvl0.n_dev)
        levels.append(lv)
        return lv, sp.subm_geom(lv)

    def residual_pair(x, w, tokens):
        lv, geom = geom_of()
        bns = [torch.nn.BatchNorm1d(c, eps=1e-3, momentum=0.01).to(cuda).train() for _ in range(2)]
        tok = sp.ResidualToken() if tokens else None
        o = sp.conv_bn(x, w[0], geom, bns[0], lv.n_dev, None, True, res_take=tok)
        return sp.conv_bn(o, w[1], geom, bns[1], lv.n_dev, x, True, res_give=tok), [tok] if tokens else []

    def fanout(x, w, tokens):
        lv, geom = geom_of()
        fan = sp.FanoutToken(2) if tokens else None
        return sp.sparse_conv(x, w[0], geom, fan_token=fan) + sp.sparse_conv(x, w[1], geom, fan_token=fan), [fan] if tokens else []

    with sp.split_scope(route.startswith("split")):
        for build in (residual_pair, fanout):
            res = _grads_with_and_without_tokens(build, x0, ws)
            for i, (p, q) in enumerate(zip(res[True], res[False])):
                err = float((p - q).abs().max() / q.abs().max())
                print(route, build.__name__, i, err)
                assert torch.isfinite(p).all() and err <= tol, (build.__name__, i, err)
        if route == "bf16_table":
            # no input gradient wanted, a token present: the conv's backward still clears what the BatchNorm left in it
            x = x0.clone()
            w = [p.clone().requires_grad_(True) for p in ws]
            y, (tok,) = residual_pair(x, w, True)
            y.backward(torch.ones_like(y))
            assert tok.dres is None and x.grad is None and all(p.grad is not None for p in w)
    if route == "bf16_halo":
        assert all(isinstance(lv._halo, nv.SubmHalo) for lv in levels)          # halo tables were built: the halo kernels ran
    elif route == "bf16_table":
        assert all(lv._halo is None for lv in levels)                            # never asked for: the table kernels ran


def _strided_route_addends(cuda, bf16):
    """test_gradient_addends_same_on_every_route for the strided input gradient (per-offset products over the output rows + u3d_tap_gather_sum, bf16 and inside the split
    scope), two-branch fan-out only, at the smallest lattice with n_out * 16 <= n_in: stride (1, 4, 4), 64 -> 64, one scene of (2, 16, 16)."""
    from uni3detr_amd import sparse as sp
    from uni3detr_amd.plugin import dense as dn
    geom, _ = dn.Lattice.conv(cuda, 1, (2, 16, 16), (1, 3, 3), (1, 4, 4), (0, 1, 1))
    assert geom.strided and geom.n_out * 16 <= geom.n_in and geom.n_in == 512
    torch.manual_seed(4)
    x0 = torch.randn(geom.n_in, 64, device=cuda).to(torch.bfloat16 if bf16 else torch.float32)
    ws = [torch.randn(1, 3, 3, 64, 64, device=cuda) * 0.05 for _ in range(2)]
    real, ran = nv.tap_gather_sum, []
    nv.tap_gather_sum = lambda *a, **k: (ran.append(k.get("addend") is not None), real(*a, **k))[1]

    def fanout(x, w, tokens):
        fan = sp.FanoutToken(2) if tokens else None
        return sp.sparse_conv(x, w[0], geom, fan_token=fan) + sp.sparse_conv(x, w[1], geom, fan_token=fan), [fan] if tokens else []

    try:
        with sp.split_scope(not bf16):
            res = _grads_with_and_without_tokens(fanout, x0, ws)
    finally:
        nv.tap_gather_sum = real
    assert len(ran) == 4                                   # two branches, with and without the token: the gather served every input gradient
    tol = 1.6e-2 if bf16 else 1e-5
    for i, (p, q) in enumerate(zip(res[True], res[False])):
        err = float((p - q).abs().max() / q.abs().max())
        print("strided", bf16, i, err)
        assert torch.isfinite(p).all() and err <= tol, (i, err)
