"""InferenceModel(sparse_levels=True) on the GPU: the affine instantiations of the halo kernels (u3d_subm_halo_conv_bf16 with a shift)
and of the direct-operand kernels (u3d_igemm_direct_affine_bf16) against the entries they are built from and against the float64
restatement of tests/test_bn_fold_sparse_cpu.py, then the model: routing, launch counts, logits against the fp32 model, refresh.

E(path) = max |path - f64| / max |f64| over live rows (the measure of tests/test_bn_fold_gpu.py); the folded path is held to
E(folded) <= 2 * E(unfolded) with E(unfolded) < 2e-2, the unfolded path being conv + u3d_bn_apply as sparse._BNRows runs it."""
import ctypes

import pytest
import torch

import projects.mmdet3d_plugin  # noqa: F401
from test_bn_fold_cpu import tiny_cfg
from test_bn_fold_gpu import EPS, _bn_params, _Case, _E, _logits, _rel
from test_bn_fold_sparse_cpu import affine_epilogue64
from test_sparse_gpu import _level
from uni3detr_amd import native as nv
from uni3detr_amd import sparse as sp
from uni3detr_amd.inference import InferenceModel

pytestmark = pytest.mark.gpu
SENT = -77.0


def _same_values(a, b):
    """torch.equal on values: +0 and -0 are the same number (relu() and `+ 0.0` may change the sign of a zero)."""
    return a.shape == b.shape and bool((a.float() == b.float()).all())


def _ref64(conv64, shift64, addend, relu):
    add = None if addend is None else addend.double().cpu().numpy()
    return torch.from_numpy(affine_epilogue64(conv64.cpu().numpy(), shift64.cpu().numpy(), add, relu)).to(conv64.device)


# ---- halo kernels -------------------------------------------------------------------------------------------------------------------
class _HaloCase:
    """A real SubM level with a device-side count below its capacity, inputs, an f32 master weight, BatchNorm parameters and the
    float64 convolutions of one (C, size); built once and shared."""
    # (points, dims, dead rows): 333 rows = 3 tiles of 128 with 300 live (the last live tile is partial); 4892 rows with 4500 live
    SIZES = {"small": (420, (4, 8, 8), 33), "large": (6000, (8, 24, 24), 392)}

    def __init__(self, c, size, dev):
        n_pts, dims, cut = self.SIZES[size]
        lvl, nbr = _level(seed=7, n_pts=n_pts, dims=dims)
        self.c, self.n_cap = c, lvl.n
        self.n = n = lvl.n - cut
        assert (size == "small" and 256 < self.n_cap <= 384 and n % 128 and abs(n - 300) <= 20) or (size == "large" and abs(n - 4500) <= 100)
        self.n_dev = nv.count_tensor(n, "cuda")
        nb = nbr.clone()
        nb[:, :n][nb[:, :n] >= n] = -1
        self.nbr = nb
        self.halo = nv.SubmHalo(nb, self.n_dev, self.n_cap)
        gen = torch.Generator().manual_seed(100 + c + n_pts)
        self.x = torch.randn(self.n_cap, c, generator=gen).to(dev).bfloat16()
        self.res = torch.randn(self.n_cap, c, generator=gen).to(dev).bfloat16()                      # the identity: bf16, unit scale
        self.x[n:] = float("nan")                                                                   # dead rows are never read
        self.res[n:] = float("nan")
        self.w = (torch.randn(27, c, c, generator=gen) / (27 * c * 0.3) ** 0.5).to(dev)              # f32 master, n-major [K][out][in]
        self.bn = _bn_params(c, gen, dev)
        self.scale = self.bn["gamma"].double() / torch.sqrt(self.bn["var"].double() + EPS)
        self.shift64 = self.bn["beta"].double() - self.bn["mean"].double() * self.scale
        self.conv64 = self._conv64()                                                                 # [n, c], live rows, unfolded weights

    def _conv64(self):
        x, w = self.x[:self.n].double(), self.w.double()
        out = torch.zeros(self.n, self.c, dtype=torch.float64, device=x.device)
        for k in range(27):
            idx = self.nbr[k, :self.n].long()
            out += (x[idx.clamp(min=0)] * (idx >= 0).unsqueeze(1)) @ w[k].t()
        return out


_HALO = {}


@pytest.fixture
def halo_case(cuda, request):
    key = request.param
    if key not in _HALO:
        _HALO[key] = _HaloCase(key[0], key[1], cuda)
    return _HALO[key]


@pytest.mark.parametrize("halo_case", [(64, "small"), (64, "large"), (128, "small"), (128, "large")], indirect=True, ids=str)
def test_halo_affine_identities_padding_and_error_bound(cuda, halo_case):
    h = halo_case
    c, n, n_cap = h.c, h.n, h.n_cap
    wp = nv.subm_halo_wpack(h.w.bfloat16())
    zero = torch.zeros(c, device=cuda)
    assert int(h.halo.tile_cnt.max()) > 40                       # max_slots = 40: some slots of every such tile come from global memory
    for ms in (0, 40):
        for add in (None, h.res):
            base = nv.subm_halo_conv(h.x, wp, h.halo, addend=add, max_slots=ms)
            assert bool(torch.isfinite(base[:n]).all())
            for relu in (0, 1):
                out = torch.full((n_cap, c), SENT, dtype=torch.bfloat16, device=cuda)
                got = nv.subm_halo_conv_affine(h.x, wp, h.halo, zero, relu, addend=add, max_slots=ms, out=out)
                want = torch.relu(base[:n]) if relu else base[:n]
                assert got is out and _same_values(got[:n], want), (ms, add is not None, relu)        # (i), (ii)
                assert bool((got[n:] == SENT).all())                                                  # (iii)
    # (iv) folded by the fold kernel from the f32 master, packed; against conv + u3d_bn_apply and the float64 restatement
    wf, sh = torch.empty((27, c, c), dtype=torch.bfloat16, device=cuda), torch.empty(c, device=cuda)
    master = h.w.permute(1, 2, 0).contiguous().view(c, c, 1, 1, 27)                                   # [Cout,Cin,kD,kH,kW]
    nv.bn_fold([(master, "oidhw", h.bn["gamma"], h.bn["beta"], h.bn["mean"], h.bn["var"], EPS, wf, sh)])
    wfp = nv.subm_halo_wpack(wf)
    invstd = torch.rsqrt(h.bn["var"] + EPS)
    for ms in (0, 40):
        for add in (None, h.res):
            ref = _ref64(h.conv64 * h.scale[None], h.shift64, None if add is None else add[:n], True)
            folded = nv.subm_halo_conv_affine(h.x, wfp, h.halo, sh, True, addend=add, max_slots=ms)
            y0 = nv.subm_halo_conv(h.x, wp, h.halo, max_slots=ms)
            unfolded = nv.bn_apply(y0, h.bn["mean"], invstd, h.bn["gamma"], h.bn["beta"], add, True, h.n_dev)
            ef, eu = _E(folded, ref, n), _E(unfolded, ref, n)
            print(f"halo{c} n={n} max_slots={ms} residual={add is not None}: E(folded) = {ef:.3e}  E(unfolded) = {eu:.3e}")
            assert eu < 2e-2
            assert ef <= 2 * eu, (ef, eu)


@pytest.mark.parametrize("c", [64, 128])
def test_halo_affine_refuses_krev_and_zero_shift_is_the_plain_conv(cuda, c):
    """The merged entry on the smallest level of the halo tests (a few 128-row tiles): an affine call with krev = 1 is U3D_ERR_ARG
    and writes nothing (the affine kernels used to zero krev silently); with a zero shift and no ReLU the affine instantiation gives
    the plain one's bits."""
    lvl, nbr = _level(seed=3, n_pts=300, dims=(8, 8, 8))
    n, live = lvl.n, int(lvl.n_dev.item())
    halo = nv.SubmHalo(nbr, lvl.n_dev, n)
    assert halo.ok and halo.kvol == 27 and halo.tiles >= 2 and 0 < live <= n
    torch.manual_seed(c)
    x = torch.randn(n, c, device=cuda).bfloat16()
    wp = nv.subm_halo_wpack((torch.randn(27, c, c, device=cuda) * 0.1).bfloat16())
    zero = torch.zeros(c, device=cuda)
    out = torch.full((n, c), SENT, dtype=torch.bfloat16, device=cuda)
    rc = nv.lib().u3d_subm_halo_conv_bf16(nv._ptr(x), nv._ptr(wp), ctypes.byref(halo.tables), c, 1, None, nv._ptr(out), None, nv._ptr(zero),
                                          0, 0, nv._stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool((out.view(torch.int16) == torch.tensor(SENT).bfloat16().view(torch.int16).item()).all())
    base = nv.subm_halo_conv(x, wp, halo)
    got = nv.subm_halo_conv_affine(x, wp, halo, zero, False)
    assert bool(torch.isfinite(base[:live]).all()) and float(base[:live].float().abs().max()) > 0
    assert torch.equal(got[:live].view(torch.int16), base[:live].view(torch.int16))


# ---- direct-operand kernels -------------------------------------------------------------------------------------------------------------
_DIRECT = {}


@pytest.mark.parametrize("cin,cout", [(16, 16), (16, 32), (32, 32), (32, 64)])
def test_direct_affine_identities_padding_and_error_bound(cuda, cin, cout):
    n = 1000
    if (cin, cout) not in _DIRECT:
        _DIRECT[(cin, cout)] = _Case(n, cin, cout, 27, True, cuda, seed=cin * 100 + cout)
    c = _DIRECT[(cin, cout)]
    live = c.live
    assert live == n - 13
    gen = torch.Generator().manual_seed(cin + cout)
    res = torch.randn(n, cout, generator=gen).to(cuda).bfloat16()
    wb = c.w.bfloat16()
    # the plain forward of this shape IS the direct-operand kernel: its rule serves the shape, no LDS-DMA tile does (channels % 64),
    # and both entries accept it - so the identities below compare one kernel family with itself
    assert nv.direct_serves(cin, cout, 27) and nv.igemm_fwd_affine_plan(n, cin, cout, 27, True) is None
    probe = torch.empty((n, cout), dtype=torch.bfloat16, device=cuda)
    for addend in (None, res):
        assert nv.lib().u3d_igemm_fwd_bf16(nv._ptr(c.x), nv._ptr(wb), nv._ptr(c.nbr), n, nv._ptr(probe), nv._ptr(c.n_dev), n, cin, cout, 27, 1,
                                           nv._ptr(addend), None, nv._stream()) == 0
    zero = torch.zeros(cout, device=cuda)
    for add in (None, res):
        base = nv.spconv_fwd(c.x, wb, c.nbr, c.n_dev, n, cout, transpose_w=True, addend=add)
        for relu in (0, 1):
            out = torch.full((n, cout), SENT, dtype=torch.bfloat16, device=cuda)
            got = nv.igemm_direct_affine(c.x, wb, c.nbr, zero, relu, c.n_dev, n, addend=add, out=out)
            want = torch.relu(base[:live]) if relu else base[:live]
            assert got is out and _same_values(got[:live], want), (add is not None, relu)             # (i), (ii)
            assert bool((got[live:] == SENT).all())                                                   # (iii)
    wf, sh = torch.empty((27, cout, cin), dtype=torch.bfloat16, device=cuda), torch.empty(cout, device=cuda)
    master = c.w.permute(1, 2, 0).contiguous().view(cout, cin, 1, 1, 27)
    nv.bn_fold([(master, "oidhw", c.bn["gamma"], c.bn["beta"], c.bn["mean"], c.bn["var"], EPS, wf, sh)])
    invstd = torch.rsqrt(c.bn["var"] + EPS)
    for add in (None, res):
        ref = _ref64(c.conv64 * c.scale[None], c.shift64, add, True)
        folded = nv.igemm_direct_affine(c.x, wf, c.nbr, sh, True, c.n_dev, n, addend=add)
        y0 = nv.spconv_fwd(c.x, wb, c.nbr, c.n_dev, n, cout, transpose_w=True, tag="spconv_fwd")
        unfolded = nv.bn_apply(y0, c.bn["mean"], invstd, c.bn["gamma"], c.bn["beta"], add, True, c.n_dev)
        ef, eu = _E(folded, ref, live), _E(unfolded, ref, live)                                       # (iv)
        print(f"direct {cin}->{cout} residual={add is not None}: E(folded) = {ef:.3e}  E(unfolded) = {eu:.3e}")
        assert eu < 2e-2
        assert ef <= 2 * eu, (ef, eu)


def test_direct_affine_refuses_a_shape_without_an_instantiation(cuda):
    n = 256
    x = torch.zeros(n, 64, dtype=torch.bfloat16, device=cuda)
    w = torch.zeros(27, 64, 64, dtype=torch.bfloat16, device=cuda)
    nbr = torch.full((27, n), -1, dtype=torch.int32, device=cuda)
    n_dev = torch.tensor([n], dtype=torch.int32, device=cuda)
    with pytest.raises(nv.U3DError, match="igemm_direct_affine_bf16"):
        nv.igemm_direct_affine(x, w, nbr, torch.zeros(64, device=cuda), 1, n_dev, n)


# ---- the model ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(cuda):
    from oracle.weights import seeded_tensor
    from uni3detr_amd.registry import build_model
    from uni3detr_amd.synth import room_scene
    model = build_model(tiny_cfg())
    model.load_state_dict({k: seeded_tensor(k, tuple(v.shape), 3) for k, v in model.state_dict().items()})
    model = model.to(cuda).eval()
    mk = lambda i, n: torch.from_numpy(room_scene(i, n)[0]).to(cuda)      # noqa: E731
    # small: the B = 2 scenes of tests/test_bn_fold_gpu.py; large: one scene whose 64- and 128-channel levels both have well over 4096
    # rows (about 27 k and 6.8 k); sparse: one scene whose wide levels stay under 4096 rows (about 2.5 k each)
    return model, dict(small=[mk(i, 9000 - 2500 * i) for i in range(2)], large=[mk(0, 20000)], sparse=[mk(0, 500)])


def _count(monkeypatch, name, calls):
    orig = getattr(nv, name)
    monkeypatch.setattr(nv, name, lambda *a, **k: calls.append(name) or orig(*a, **k))


def _wide_blocks(model):
    """[(stage index, SparseBasicBlock)] of the 64- / 128- / 256-channel stages."""
    from uni3detr_amd.plugin.sparse_encoder import SparseBasicBlock
    return [(si, m) for si, stage in enumerate(model.pts_middle_encoder.encoder_layers) for m in stage
            if isinstance(m, SparseBasicBlock) and m.conv1.cin % 64 == 0]


def test_model_routing_and_launch_counts(scene, monkeypatch):
    model, pts = scene
    model.set_precision("bf16")
    inf = InferenceModel(model, sparse_levels=True)
    n_bn = sum(isinstance(x, torch.nn.modules.batchnorm._BatchNorm) for x in model.modules())
    assert len(inf.unfolded) == 3 and len(inf.folded) == n_bn - 3 == 13 + 16 + 2
    wide = _wide_blocks(model)
    assert len(wide) == 4
    calls = []
    for name in ("bn_apply", "subm_halo_conv_affine", "igemm_direct_affine", "igemm_fwd_affine"):
        _count(monkeypatch, name, calls)
    enc = model.pts_middle_encoder
    for key in ("large", "small", "sparse"):
        calls.clear()
        if key == "sparse":             # 500 points: the feature extractor alone (the head's 300 FPS queries are not this test's subject)
            with torch.no_grad(), inf.scope():
                model.stage_features(model.stage_voxelize(pts[key]))
        else:
            inf.extract_pts_feat(pts[key])
        assert sp._FOLD[0] is None
        # stage si (0-based) runs on level si: rows of the level each wide block ran on
        rows = [int(enc.last_level_counts[si]) for si, _ in wide]
        served = [r >= 4096 for r in rows]
        fell_back = sum(not s for s in served)                  # one conv2 per wide block on a level the halo kernels do not serve
        print(f"{key}: wide-block level rows {rows}, halo-affine calls {calls.count('subm_halo_conv_affine')}, "
              f"bn_apply calls {calls.count('bn_apply')}")
        assert calls.count("subm_halo_conv_affine") == 2 * sum(served)
        assert calls.count("bn_apply") == len(inf.unfolded) + fell_back
        assert calls.count("igemm_direct_affine") == 2 * 4 + 2                                      # the narrow blocks and strided convs
        # LDS-DMA affine: the default mode's 13 layers + conv1 of every wide block that fell back
        assert calls.count("igemm_fwd_affine") == 13 + fell_back
        if key == "large":
            assert all(served) and calls.count("subm_halo_conv_affine") == 8 and calls.count("bn_apply") == len(inf.unfolded)
        if key == "sparse":
            assert not any(served) and calls.count("bn_apply") == len(inf.unfolded) + 4
    # the unfolded forward runs one apply pass per BatchNorm, and leaves no scope behind
    calls.clear()
    with torch.no_grad():
        model.extract_pts_feat(pts["small"])
    assert calls.count("bn_apply") == n_bn and calls.count("subm_halo_conv_affine") == 0 and sp._FOLD[0] is None
    # a call that raises inside the scope closes it too
    monkeypatch.setattr(nv, "igemm_direct_affine", lambda *a, **k: (_ for _ in ()).throw(RuntimeError("boom")))
    with pytest.raises(RuntimeError, match="boom"):
        inf.extract_pts_feat(pts["small"])
    assert sp._FOLD[0] is None


@pytest.mark.parametrize("key", ["small", "large"])
def test_model_logits_sparse_levels_vs_unfolded_against_fp32(scene, key):
    """Deviation = relative L2 of the head's class / box logits from the same model under set_precision('fp32'), the measure and gate of
    test_model_logits_folded_vs_unfolded_against_fp32: folded <= 2 x unfolded."""
    model, pts = scene
    ref = _logits(model.set_precision("fp32"), pts[key])
    model.set_precision("bf16")
    unf = _logits(model, pts[key])
    inf = InferenceModel(model, sparse_levels=True)
    fol = _logits(model, pts[key], inf)
    assert sp._FOLD[0] is None
    for name, r, u, f in zip(("cls", "box"), ref, unf, fol):
        du, df = _rel(u, r), _rel(f, r)
        print(f"{key} {name} logits: sparse_levels {df:.3e}  unfolded {du:.3e}")
        assert df <= 2 * du, (name, df, du)


def test_model_batched_tail_and_refresh(scene):
    model, allpts = scene
    pts = allpts["small"]
    model.set_precision("bf16")
    inf = InferenceModel(model, sparse_levels=True)
    # refresh(): the fold and one pack launch per channel count; the plans stay while nothing moved
    assert [p.c for p in inf._packs] == [64, 128] and [p.n for p in inf._packs] == [4, 4]
    table, packs = inf._table, inf._packs
    inf.refresh()
    assert inf._table is table and inf._packs is packs
    det = inf.simple_test_batched(None, pts, on_device=True)
    assert sp._FOLD[0] is None
    K = det.boxes.shape[1]
    cnt = det.count.cpu().tolist()
    assert det.boxes.is_cuda and len(cnt) == 2 and all(0 <= c <= K for c in cnt)
    for b, c in enumerate(cnt):
        assert not bool(det.boxes[b, c:].any()) and not bool(det.scores[b, c:].any()) and not bool(det.labels[b, c:].any())
    # running statistics of a sparse-level BatchNorm changed in place: the folded buffers, and so the output, move only at refresh().
    # The BatchNorm of the strided 32 -> 64 conv (direct-operand affine kernel): the whole 64-channel level passes through it, with no
    # identity branch around it.  "Does not move" = within 1e-2, the bound tests/test_bn_fold_gpu.py puts on two forwards of the same
    # state (reordered f32 sums, ~1e-3); "moves" = beyond that same bound; and after refresh() the output is that of an InferenceModel
    # wrapped afresh around the changed statistics, to the same 1e-2.  (How far four running standard deviations move the output is
    # not asserted: the seeded running statistics are not the statistics of these activations, so the step has no known size in
    # units of the features.)
    bn = dict(model.named_modules())["pts_middle_encoder.encoder_layers.encoder_layer2.2.1"]
    ent = inf._by_bn[id(bn)]
    assert ent.w_folded.shape == (27, 64, 32) and ent.sparse_level and ent.route == "direct" and ent.w_packed is None
    shift = ent.shift
    delta = 4 * bn.running_var.sqrt()
    a, s0 = inf.extract_pts_feat(pts)[0].double(), shift.clone()
    bn.running_mean.add_(delta)
    b, s1 = inf.extract_pts_feat(pts)[0].double(), shift.clone()
    inf.refresh()
    c, s2 = inf.extract_pts_feat(pts)[0].double(), shift.clone()
    fresh = InferenceModel(model, sparse_levels=True).extract_pts_feat(pts)[0].double()
    bn.running_mean.sub_(delta)
    inf.refresh()
    print(f"refresh: without {_rel(b, a):.3e}, with {_rel(c, a):.3e}, against a fresh wrapper {_rel(c, fresh):.3e}")
    assert torch.equal(s0, s1) and not torch.equal(s1, s2)
    assert torch.allclose(shift, s0, atol=1e-5)                        # ((m + d) - d is m up to an f32 rounding)
    assert _rel(b, a) <= 1e-2 and _rel(c, a) > 1e-2 and _rel(c, fresh) <= 1e-2
    # a halo-served block: its packed weights are rewritten by the same refresh()
    bn2 = dict(model.named_modules())["pts_middle_encoder.encoder_layers.encoder_layer3.0.bn1"]
    e2 = inf._by_bn[id(bn2)]
    assert e2.sparse_level and e2.route == "halo" and e2.w_packed.shape == (27, 64, 64)
    p0 = e2.w_packed.clone()
    bn2.running_var.mul_(1.7)
    assert torch.equal(e2.w_packed.view(torch.int16), p0.view(torch.int16))
    inf.refresh()
    assert not torch.equal(e2.w_packed.view(torch.int16), p0.view(torch.int16))
    assert torch.equal(e2.w_packed.view(torch.int16), nv.subm_halo_wpack(e2.w_folded).view(torch.int16))
    bn2.running_var.div_(1.7)
    inf.refresh()
