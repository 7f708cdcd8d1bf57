"""GPU: test-time augmentation behind the batched tail.  The merge over the padded layout (u3d_tta_merge_padded) bit for bit against
the ragged entry on the compacted rows - itself pinned to the NumPy restatement by tests/test_tta_gpu.py -, its zero tail and `off`, the
global-memory path, capture and replay, the error codes; then InferenceStep(views=2) on the tiny model of tests/test_infer_step_gpu.py
(that file's scenes, seed discipline and yardstick: a replay's logits within 2 x the eager folded forward's deviation from fp32), the
eager on-device path against aug_test, and the dataset loop with a partial and a repaired batch.

Every compared forward starts from the same torch.manual_seed: the head draws random query points per eval forward (that file's header)."""
import numpy as np
import pytest
import torch

import projects.mmdet3d_plugin  # noqa: F401
import tta_ref as R
from test_bn_fold_cpu import tiny_cfg
from test_tta_cpu import random_views
from test_varlen_gpu import _no_host_sync
from uni3detr_amd import datapath as dp
from uni3detr_amd import native as nv
from uni3detr_amd import static_batch as sb
from uni3detr_amd import testing, tta
from uni3detr_amd.inference import InferenceModel, InferenceStep

pytestmark = pytest.mark.gpu
DOUBLE_FLIP = [(0.0, 1.0, False, False), (0.0, 1.0, False, True), (0.0, 1.0, True, False), (0.0, 1.0, True, True)]
ROT_SCALE = [(0.0, 1.0, False, False), (0.3, 1.05, False, True), (0.0, 1.0, True, False), (-0.2, 0.95, True, True)]
NAMES = ("boxes", "scores", "labels", "count", "off")


def _metas(params):
    return [dict(rot_degree=r, pcd_scale_factor=s, pcd_horizontal_flip=h, pcd_vertical_flip=v) for r, s, h, v in params]


# ---- the merge ---------------------------------------------------------------------------------------------------------------------
def _pad(cuda, views, K, dim, ncls, rng):
    """views: per view (boxes [n <= K, dim], scores, labels) numpy -> the padded DetBatch; the rows past each count hold what must
    never be read: NaN scores, huge boxes and labels that look valid"""
    V = len(views)
    boxes = np.full((V, K, dim), 1e30, np.float32)
    scores = np.full((V, K), np.nan, np.float32)
    labels = rng.integers(0, ncls, (V, K)).astype(np.int32)
    count = np.array([len(v[1]) for v in views], np.int32)
    for i, (b, s, l) in enumerate(views):
        boxes[i, :count[i]], scores[i, :count[i]], labels[i, :count[i]] = np.asarray(b).reshape(-1, dim), s, l
    t = lambda a: torch.from_numpy(a).to(cuda)                                            # noqa: E731
    off = torch.full((V + 1,), -1, dtype=torch.int32, device=cuda)                        # (not read by the merge)
    return nv.DetBatch(t(boxes), t(scores), t(labels), t(count), off)


def _ragged(cuda, views, tab, A, coord, ncls, dim, **kw):
    """the reference: native.tta_merge on the compacted rows -> the five tensors of a DetBatch (zero tail, off), host numpy"""
    lens = [len(v[1]) for v in views]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64).tolist()
    cat = lambda k, dt: torch.from_numpy(np.concatenate([np.asarray(v[k], dt).reshape((-1, dim) if k == 0 else (-1,)) for v in views])).to(cuda)  # noqa: E731
    ob, os_, ol, oc = nv.tta_merge(cat(0, np.float32), cat(1, np.float32), cat(2, np.int32), off, tab, A, coord, ncls, **kw)
    ob, os_, ol, oc = ob.cpu().numpy(), os_.cpu().numpy(), ol.cpu().numpy(), oc.cpu().numpy()
    live = np.arange(ob.shape[1])[None, :] < oc[:, None]
    return (np.where(live[..., None], ob, 0).astype(np.float32), np.where(live, os_, 0).astype(np.float32), np.where(live, ol, 0).astype(np.int32),
            oc, np.concatenate([[0], np.cumsum(oc)]).astype(np.int32))


def _preset(out):
    for name in NAMES:
        getattr(out, name).fill_(-1)
    return out


def _assert_equal(got, want, what=""):
    for name, w in zip(NAMES, want):
        g = getattr(got, name).cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name, np.argwhere(g != w)[:6].tolist())


def _cut_views(rng, B, params, coord, dim, K, ncls):
    """B samples of len(params) views: K candidates each, cut to random counts of which one is 0 and one is K in every draw"""
    A = len(params)
    counts = rng.integers(0, K + 1, B * A)
    where = rng.choice(B * A, 2, replace=False)
    counts[where[0]], counts[where[1]] = 0, K
    flat = [v for _ in range(B) for v in random_views(rng, params, coord, dim=dim, n=(K, K), ncls=ncls)]
    return [(b[:c], s[:c], l[:c].astype(np.int32)) for (b, s, l), c in zip(flat, counts)], counts


@pytest.mark.parametrize("coord", [R.DEPTH, R.LIDAR])
@pytest.mark.parametrize("dim", [7, 9])
def test_padded_merge_equals_ragged_bit_for_bit(cuda, coord, dim):
    rng = np.random.default_rng(100 + dim + 10 * coord)
    B, A, K, ncls = 3, 4, 8, 4
    tab = tta.view_params(_metas(ROT_SCALE) * B, cuda)
    out = None
    for draw in range(3):
        views, counts = _cut_views(rng, B, ROT_SCALE, coord, dim, K, ncls)
        assert 0 in counts and K in counts
        det = _pad(cuda, views, K, dim, ncls, rng)
        if out is None:
            out = nv.tta_merge_padded(det, tab, A, coord, ncls)                          # allocates; every later call reuses it
        got = nv.tta_merge_padded(det, tab, A, coord, ncls, out=_preset(out))
        assert got is out and tuple(out.boxes.shape) == (B, 500, dim)
        _assert_equal(got, _ragged(cuda, views, tab, A, coord, ncls, dim), f"draw {draw}")
        assert int(got.count.sum()) > 0
    if coord == R.LIDAR and dim == 7:
        # this draw against the restatement itself (tolerances: tests/test_tta_gpu.py _assert_same)
        cnt = got.count.tolist()
        for b in range(B):
            rb, rs, rl = R.merge(views[b * A:(b + 1) * A], ROT_SCALE, coord)
            gb, gs, gl = (t[b, :cnt[b]].cpu().numpy() for t in (got.boxes, got.scores, got.labels))
            np.testing.assert_array_equal(gl, rl)
            np.testing.assert_allclose(gs, rs, rtol=1e-6)
            cols = [c for c in range(dim) if c != 6]
            np.testing.assert_allclose(gb[:, cols], rb[:, cols], rtol=1e-6, atol=1e-6 * 30.0)
            assert R.yaw_close(gb[:, 6], rb[:, 6], 1e-5).all()


def test_padded_merge_edge_cases(cuda):
    """in ONE call: samples whose views are all empty in front of, between and behind the others, more survivors than max_num = 5,
    NaN / inf scores inside the counted rows, label gaps"""
    rng = np.random.default_rng(11)
    P, ncls, M = DOUBLE_FLIP, 7, 5
    empty = [(np.zeros((0, 7), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32)) for _ in P]
    single = [(b, s, l.astype(np.int32)) for b, s, l in random_views(rng, P, R.LIDAR, n=(6, 12), ncls=1, extent=30.0)]
    gaps = [(b, s.copy(), (l * 3).astype(np.int32)) for b, s, l in random_views(rng, P, R.LIDAR, ncls=3)]
    gaps[1][1][0] = np.nan
    gaps[2][1][-1] = np.inf
    views = empty + single + empty + gaps + empty
    K = max(len(v[1]) for v in views)
    tab = tta.view_params(_metas(P) * 5, cuda)
    det = _pad(cuda, views, K, 7, ncls, rng)
    out = _preset(nv.tta_merge_padded(det, tab, 4, R.LIDAR, ncls, max_num=M))
    got = nv.tta_merge_padded(det, tab, 4, R.LIDAR, ncls, max_num=M, out=out)
    _assert_equal(got, _ragged(cuda, views, tab, 4, R.LIDAR, ncls, 7, max_num=M))
    cnt = got.count.tolist()
    assert cnt[0] == cnt[2] == cnt[4] == 0 and cnt[1] == M and cnt[3] > 0          # `single` had more than max_num survivors
    assert len(R.merge(single, P, R.LIDAR)[2]) > M
    assert bool(torch.isfinite(got.scores).all())
    assert set(got.labels[3, :cnt[3]].tolist()) <= {0, 3, 6}


def test_padded_merge_global_path(cuda):
    """views * K = 2400 > TTA_LDS_CAP: the mask / sweep pair is launched, and one class holds more candidates than the LDS path takes
    (a grid of unit squares, every second one duplicated 0.2 m off - tests/test_tta_gpu.py); a small second class, served by the LDS
    path, fills the rest of the 2 x 1200 rows"""
    rng = np.random.default_rng(5)
    A, K = 2, 1200
    g = np.stack(np.meshgrid(np.arange(40), np.arange(40)), -1).reshape(-1, 2).astype(np.float32)[:1574] * 1.5
    base = np.concatenate([g, np.zeros((len(g), 1)), np.ones((len(g), 3)), np.zeros((len(g), 1))], 1).astype(np.float32)
    shifted = base[::2].copy()
    shifted[:, 0] += 0.2
    big = np.concatenate([base, shifted])
    n_small = A * K - len(big)
    assert len(big) > nv.TTA_LDS_CAP and 0 < n_small < 64
    small = base[:n_small].copy()
    small[:, 1] += 0.1
    boxes = np.concatenate([big, small])
    labels = np.concatenate([np.zeros(len(big), np.int32), np.ones(n_small, np.int32)])
    scores = (rng.permutation(len(boxes)).astype(np.float32) + 1) / len(boxes)
    views = [(boxes[:K], scores[:K], labels[:K]), (boxes[K:], scores[K:], labels[K:])]
    tab = tta.view_params(_metas([(0.0, 1.0, False, False)] * 2), cuda)
    det = _pad(cuda, views, K, 7, 2, rng)
    got = nv.tta_merge_padded(det, tab, A, R.LIDAR, 2, max_num=5000)
    _assert_equal(got, _ragged(cuda, views, tab, A, R.LIDAR, 2, 7, max_num=5000))
    assert nv.TTA_LDS_CAP // 2 < int(got.count[0]) < len(big)


def test_padded_merge_is_capturable_and_zeroes_stale_rows(cuda):
    rng = np.random.default_rng(31)
    B, A, K, ncls, dim = 2, 4, 8, 4, 7
    tab = tta.view_params(_metas(ROT_SCALE) * B, cuda)
    first = [v for _ in range(B) for v in random_views(rng, ROT_SCALE, R.LIDAR, n=(K, K), ncls=ncls)]
    first = [(b, s, l.astype(np.int32)) for b, s, l in first]
    second = [(b[:c], s[:c], l[:c]) for (b, s, l), c in zip(first[::-1], [1, 0, 2, 0, 0, 1, 0, 0])]        # far fewer rows: stale ones must go
    contents = [_pad(cuda, v, K, dim, ncls, rng) for v in (first, second)]
    static = _pad(cuda, first, K, dim, ncls, rng)
    out = nv.tta_merge_padded(static, tab, A, R.LIDAR, ncls)
    call = lambda: nv.tta_merge_padded(static, tab, A, R.LIDAR, ncls, out=out)                              # noqa: E731
    graph = sb.capture_graph(call, sb.warm_up(call, 2))
    torch.cuda.synchronize()
    counts = []
    for src in contents:
        for name in NAMES[:4]:
            getattr(static, name).copy_(getattr(src, name))
        graph.replay()
        torch.cuda.synchronize()
        with _no_host_sync():
            eager = nv.tta_merge_padded(src, tab, A, R.LIDAR, ncls)
        torch.cuda.synchronize()
        _assert_equal(out, [getattr(eager, n).cpu().numpy() for n in NAMES])
        counts.append(out.count.tolist())
        live = torch.arange(500, device=cuda)[None, :] < out.count[:, None]
        assert not bool(out.boxes[~live].any()) and not bool(out.scores[~live].any()) and not bool(out.labels[~live].any())
    assert all(c2 < c1 for c1, c2 in zip(*counts)) and sum(counts[1]) > 0


def test_padded_merge_refuses_bad_arguments(cuda):
    z = lambda *s, dt=torch.float32: torch.full(s, -1, dtype=dt, device=cuda)               # noqa: E731
    p, I32 = nv._ptr, torch.int32
    B, A, K, D, C, M = 2, 2, 4, 7, 3, 6
    bx, sc, lb, ct, pr = z(B * A, K, D), z(B * A, K), z(B * A, K, dt=I32), z(B * A, dt=I32), z(B * A, 9)
    outs = [z(B, M, D), z(B, M), z(B, M, dt=I32), z(B, dt=I32), z(B + 1, dt=I32)]
    need = int(nv.lib().u3d_tta_merge_padded_workspace(B, A, K, D, C))
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=cuda)

    def call(batch=B, views=A, K=K, dim=D, coord=1, ncls=C, max_num=M, wsb=need, null=None):
        ptrs = dict(boxes=p(bx), scores=p(sc), labels=p(lb), count=p(ct), params=p(pr), ws=p(ws), ob=p(outs[0]), os=p(outs[1]), ol=p(outs[2]),
                    oc=p(outs[3]), oo=p(outs[4]))
        if null:
            ptrs[null] = None
        return nv.lib().u3d_tta_merge_padded(ptrs["boxes"], ptrs["scores"], ptrs["labels"], ptrs["count"], batch, views, K, dim,
                                             ptrs["params"], coord, ncls, 0.1, max_num, ptrs["ws"], wsb, ptrs["ob"], ptrs["os"], ptrs["ol"],
                                             ptrs["oc"], ptrs["oo"], nv._stream())

    ARG, WORKSPACE = -1, -4
    for name in ("boxes", "scores", "labels", "count", "params", "ws", "ob", "os", "ol", "oc", "oo"):
        assert call(null=name) == ARG, name
    for kw in (dict(batch=0), dict(views=0), dict(K=0), dict(dim=8), dict(coord=2), dict(ncls=0), dict(max_num=0)):
        assert call(**kw) == ARG, kw
    big = nv.DET_TAIL_MAX_K
    for kw in (dict(batch=65536), dict(K=big + 1), dict(max_num=big + 1), dict(views=65, K=big)):      # 65 * 8192 rows: the sweep's LDS
        assert call(**kw) == nv.U3D_ERR_UNSUPPORTED, kw
    assert call(wsb=need - 1) == WORKSPACE
    assert int(nv.lib().u3d_tta_merge_padded_workspace(B, A, K, 8, C)) == -1 and int(nv.lib().u3d_tta_merge_padded_workspace(65536, A, K, D, C)) == -1
    torch.cuda.synchronize()
    assert all(bool((t == -1).all()) for t in outs)                                       # refused before any launch: nothing written
    det = nv.DetBatch(bx, sc, lb, ct, None)
    with pytest.raises(nv.U3DError, match="whole number"):
        nv.tta_merge_padded(det, z(B * A, 9), 3, 1, C)
    with pytest.raises(nv.U3DError, match="params"):
        nv.tta_merge_padded(det, z(B * A, 8), A, 1, C)
    with pytest.raises(nv.U3DError, match="same shapes"):
        nv.tta_merge_padded(det, pr, A, 1, C, max_num=M + 1, out=nv.tta_merge_padded(det, pr, A, 1, C, max_num=M))


# ---- the step --------------------------------------------------------------------------------------------------------------------------
B, A, P = 2, 2, 10240
SEED = 77


def _scenes(cuda, ids_sizes):
    from uni3detr_amd.synth import room_scene
    out = [room_scene(i, n) for i, n in ids_sizes]
    return ([torch.from_numpy(o[0]).to(cuda) for o in out], [torch.from_numpy(o[1]).to(cuda) for o in out],
            [torch.from_numpy(o[2]).to(cuda) for o in out])


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _logits(outs):
    return outs["all_cls_scores"].double().clone(), outs["all_bbox_preds"].double().clone()


def _clone(det):
    return [getattr(det, n).clone() for n in NAMES]


def _same(x, y):
    return all(torch.equal(a, b) for a, b in zip(x, y))


class _World:
    """Model, expanded batches, the fp32 reference logits and two captured views=2 steps: built once, shared, left unchanged."""

    def __init__(self, cuda):
        from oracle.weights import seeded_tensor
        from uni3detr_amd.registry import build_model
        cfg = tiny_cfg()
        model = build_model(cfg)
        model.load_state_dict({k: seeded_tensor(k, tuple(v.shape), 3) for k, v in model.state_dict().items()})
        self.model = model.to(cuda).eval()
        self.num_classes = int(model.pts_bbox_head.num_classes)
        pc = list(cfg["pts_voxel_layer"]["point_cloud_range"])
        inner = [dict(type="GlobalRotScaleTrans", rot_range=[0, 0], scale_ratio_range=[1.0, 1.0], translation_std=[0, 0, 0]),
                 dict(type="RandomFlip3D"), dict(type="PointsRangeFilter", point_cloud_range=pc)]
        self.pipe = dp.DevicePipeline([dict(type="MultiScaleFlipAug3D", img_scale=(1333, 800), pts_scale_ratio=1, flip=True,
                                            pcd_horizontal_flip=True, transforms=inner)])
        self.a = self.expand(_scenes(cuda, [(0, 9000), (1, 6500)])[0])                # B = 2 samples of different point counts
        self.b = self.expand(_scenes(cuda, [(5, 7000), (6, 8200)])[0])
        assert self.a["tta_views"] == A and tuple(self.a["tta_params"].shape) == (B * A, 9)
        self.a_views = list(dp.unpack_batch(self.a)[0])                                 # scene-major, view-minor
        self.model.set_precision("fp32")
        with torch.no_grad():
            feat, fps = self.model.extract_pts_feat(self.a_views)
            torch.manual_seed(SEED)
            self.ref = _logits(self.model.pts_bbox_head(feat, None, fps))
        self.model.set_precision("bf16")
        self.inf = InferenceModel(self.model)
        torch.manual_seed(SEED)
        self.eager = self.deviation(_logits(self.inf.head_outputs(self.a_views)))     # (cls, box) of the eager folded forward
        self.step = InferenceStep(self.inf, batch_size=B, point_capacity=P, views=A)
        self.counts, self.caps = self.step.capture(batches=[self.a, self.b], margin=1.25, warmup=2)
        # five small samples and a step sized to them at margin 1.0: the dense batch `a` overflows it
        self.small, self.small_gt, self.small_lab = _scenes(cuda, [(7, 1200), (8, 1000), (9, 1100), (10, 900), (11, 1300)])
        self.dense_gt, self.dense_lab = _scenes(cuda, [(0, 9000), (1, 6500)])[1:]
        self.tight = InferenceStep(self.inf, batch_size=B, point_capacity=P, views=A)
        last = self.expand(self.small[4:5])                                            # a partial batch: run()'s list form, padded there
        self.tight.capture(batches=[self.expand(self.small[0:2]), self.expand(self.small[2:4]),
                                    (list(dp.unpack_batch(last)[0]), last["tta_params"])], margin=1.0, warmup=1)

    def expand(self, pts):
        return self.pipe(dp.pack_batch(list(pts)))

    def deviation(self, logits):
        return tuple(_rel(x, r) for x, r in zip(logits, self.ref))


@pytest.fixture(scope="module")
def world(cuda):
    return _World(cuda)


def _run(step, batch, **kw):
    torch.manual_seed(SEED)
    return step.run(batch, **kw)


def test_feeder_side_expansion_is_what_the_step_takes(world):
    """a pipeline with the TTA block yields the expanded dict as it is: B * A scenes, the view table on the device, Depth coordinates"""
    a = world.a
    assert a["scene_off"].numel() == B * A + 1 and a["tta_params"].is_cuda and a["tta_params"].dtype == torch.float32
    assert world.step.coord == tta.DEPTH and world.step.views == A and world.step.batch_size == B
    assert a["tta_params"][:, 0].tolist() == [0.0, 1.0] * B                            # view-minor: plain, horizontally flipped


def test_replay_tail_and_merge_are_exact(world):
    step = world.step
    det = _run(step, world.a)
    assert int(step.valid) == 1 and det is step.det and det.valid is step.valid
    assert tuple(step.view_det.boxes.shape[:1]) == (B * A,) and tuple(det.boxes.shape[:2]) == (B, 500)
    with torch.no_grad(), step.inf.scope():
        tail = step.model.pts_bbox_head.get_bboxes_batched(step.head_outs, None)
    assert _same(_clone(tail), _clone(step.view_det))
    want = nv.tta_merge_padded(step.view_det, step.tta_params, A, step.coord, world.num_classes, 0.1, 500)
    nv.det_gate(want, torch.zeros(1, device=det.boxes.device), torch.full((1,), B, dtype=torch.int32, device=det.boxes.device))
    for name in NAMES:
        assert torch.equal(getattr(det, name), getattr(want, name)), name
    cnt = det.count.tolist()
    assert min(cnt) > 0 and det.off.tolist() == [0, cnt[0], cnt[0] + cnt[1]]
    assert torch.equal(step.tta_params, world.a["tta_params"])


def test_replay_head_outputs_within_twice_the_eager_deviation(world):
    _run(world.step, world.a)
    got = world.deviation(_logits(world.step.head_outs))
    for what, g, e in zip(("cls", "box"), got, world.eager):
        print(f"views=2 {what} logits: replay {g:.3e}  eager {e:.3e}")
    for what, g, e in zip(("cls", "box"), got, world.eager):
        assert g <= 2 * e, (what, g, e)


def test_eager_on_device_path_equals_aug_test(world):
    """the same exact-size folded forward under the same seed: the padded merge behind get_bboxes_batched against the ragged merge
    (aug_test(batched_tail=True), through the InferenceModel so that both run the folded route)"""
    inf = world.inf
    torch.manual_seed(SEED)
    got = inf.aug_test_batched(world.a, on_device=True)
    assert isinstance(got, nv.DetBatch) and got.boxes.is_cuda
    points, metas = dp.tta_forward_inputs(world.a)
    torch.manual_seed(SEED)
    want = inf.aug_test(points, metas, batched_tail=True)
    assert len(want) == B and sum(w["scores_3d"].shape[0] for w in want) > 0
    for (gb, gs, gl), w in zip(got.to_list(), want):
        assert torch.equal(gb.cpu(), w["boxes_3d"]) and torch.equal(gs.cpu(), w["scores_3d"]) and torch.equal(gl.cpu(), w["labels_3d"])
    # the host format, and the forward_test shape as input
    torch.manual_seed(SEED)
    res = inf.aug_test_batched(points, metas)
    assert [set(r) for r in res] == [{"boxes_3d", "scores_3d", "labels_3d"}] * B and not res[0]["boxes_3d"].is_cuda
    assert all(torch.equal(r["scores_3d"], w["scores_3d"]) and r["labels_3d"].dtype == torch.long for r, w in zip(res, want))


def test_inputs_are_read(world):
    step = world.step
    a1 = _clone(_run(step, world.a))
    b1 = _clone(_run(step, world.b))
    a2 = _clone(_run(step, world.a))
    assert not _same(a1, b1) and not torch.equal(a1[1], b1[1])
    assert torch.equal(step.tta_params, world.a["tta_params"]) and int(a2[3].sum()) > 0


def test_packed_dict_runs_without_host_sync(world):
    step = world.step
    step.run(world.b)
    torch.cuda.synchronize()
    with _no_host_sync():
        det = step.run(world.b)
    torch.cuda.synchronize()
    assert int(step.valid) == 1 and int(det.count.sum()) > 0
    # what the host knows without a read, it checks
    with pytest.raises(ValueError, match="tta_views"):
        step.run(dict(world.b, tta_views=4))
    with pytest.raises(ValueError, match="scenes"):
        step.run(world.expand(_scenes(det.boxes.device, [(5, 3000)])[0]))
    with pytest.raises(ValueError, match="tta_params"):
        step.run(dict(world.b, tta_params=world.b["tta_params"][:2]))
    with pytest.raises(ValueError, match="coordinates"):
        step.run(dict(world.b, box_type_3d="LiDAR"))


def test_partial_batch(world):
    step = world.step
    views, tab = world.a_views[:A], world.a["tta_params"][:A].contiguous()
    full = _clone(_run(step, views + views, tta_params=tab.repeat(2, 1)))             # the same views in front, sample 0 again behind
    det = _run(step, views, tta_params=tab)
    cnt = det.count.tolist()
    assert int(step.valid) == 1 and int(step.n_live) == 1 and cnt[0] > 0 and cnt[1] == 0
    assert not bool(det.boxes[1].any()) and not bool(det.scores[1].any()) and not bool(det.labels[1].any())
    assert det.off.tolist() == [0, cnt[0], cnt[0]]
    assert cnt[0] == int(full[3][0]) and all(torch.equal(getattr(det, n)[0], f[0]) for n, f in zip(NAMES[:3], full))
    torch.manual_seed(SEED)
    res = step.results(views, tta_params=tab)
    assert len(res) == 1 and res[0]["boxes_3d"].shape[0] == cnt[0] and not res[0]["boxes_3d"].is_cuda and step.fallbacks == 0
    with pytest.raises(ValueError, match="tta_params"):
        step.run(views)
    with pytest.raises(ValueError, match="scenes"):
        step.run(world.a_views[:3], tta_params=world.a["tta_params"][:3].contiguous())


def test_invalid_replay_is_gated_and_falls_back(world, monkeypatch):
    step, inf, enc = world.tight, world.inf, world.model.pts_middle_encoder
    inf.extract_pts_feat(world.a_views)
    dense_counts = [int(c) for c in enc.last_level_counts]
    assert any(c > cap for c, cap in zip(dense_counts[1:], step._caps))        # the dense batch really exceeds what was captured
    det = step.run(world.a)
    assert int(step.valid) == 0 and det.count.tolist() == [0, 0] and det.off.tolist() == [0, 0, 0]
    assert not bool(det.boxes.any()) and not bool(det.scores.any()) and not bool(det.labels.any())
    before = step.fallbacks
    seen, orig = [], inf.aug_test_batched
    monkeypatch.setattr(inf, "aug_test_batched", lambda *a, **k: seen.append(torch.cuda.get_rng_state(det.boxes.device)) or orig(*a, **k))
    res = step.results(world.a)
    monkeypatch.undo()
    assert len(seen) == 1 and step.fallbacks == before + 1 and len(res) == B
    torch.cuda.set_rng_state(seen[0], det.boxes.device)
    want = inf.aug_test_batched(world.a)
    assert [r["scores_3d"].shape[0] for r in res] == [w["scores_3d"].shape[0] for w in want] and res[0]["scores_3d"].shape[0] > 0
    det = step.run(world.expand(world.small[0:2]))                                    # a following in-capacity batch is valid again
    assert int(step.valid) == 1 and int(det.count.sum()) > 0


def test_single_view_step_holds_no_view_buffers(world):
    step = InferenceStep(world.inf, batch_size=B, point_capacity=P)
    pts = world.small[0:2]
    step.capture(batches=[pts], warmup=1)
    det = _run(step, pts)
    assert step.views == 1 and step.view_det is None and step.tta_params is None and step.coord is None
    assert int(step.valid) == 1 and int(det.count.sum()) > 0 and tuple(step.pts["scene_off"].shape) == (B + 1,)
    with torch.no_grad(), step.inf.scope():
        want = step.model.pts_bbox_head.get_bboxes_batched(step.head_outs, None)
    assert _same(_clone(det), _clone(want))


# ---- the dataset loop ----------------------------------------------------------------------------------------------------------------
def test_dataset_loop_with_a_partial_and_a_repaired_batch(world, cuda):
    """5 samples in batches of 2 x 2 views: the middle batch overflows the captured capacities and is repaired through reload, the
    last one is partial.  on_batch seeds by batch, in the loop and in the per-batch reference"""
    from uni3detr_amd.det_store import DetStore
    from uni3detr_amd.evaluation import IndoorEvaluator
    step, inf = world.tight, world.inf
    small = world.small
    dense = [world.a_views[0], world.a_views[A]]                                      # the un-flipped views = the raw dense scenes
    samples = [small[0:2], dense, small[4:5]]
    gts = world.small_gt[0:2] + world.dense_gt + world.small_gt[4:5]
    labs = world.small_lab[0:2] + world.dense_lab + world.small_lab[4:5]
    batches = [world.expand(s) for s in samples]
    assert batches[2]["scene_off"].numel() == A + 1
    # the per-batch sequence: step.results(), the fallback's forward seeded like the replay's
    orig = inf.aug_test_batched
    want, before = [], step.fallbacks
    try:
        for i, batch in enumerate(batches):
            inf.aug_test_batched = lambda *a, _i=i, **kw: torch.manual_seed(SEED + _i) and orig(*a, **kw)
            torch.manual_seed(SEED + i)
            if batch["scene_off"].numel() - 1 < B * A:
                want += step.results(list(dp.unpack_batch(batch)[0]), tta_params=batch["tta_params"])
            else:
                want += step.results(batch)
    finally:
        del inf.aug_test_batched
    assert step.fallbacks == before + 1 and len(want) == 5
    store = DetStore(5, step.tta_max_num, 7, cuda)
    with pytest.raises(RuntimeError, match="batch 1 .*no reload"):
        testing.test_dataset(step, iter(batches), DetStore(5, step.tta_max_num, 7, cuda), on_batch=lambda i: torch.manual_seed(SEED + i))
    testing.test_dataset(step, iter(batches), store, reload=lambda i: batches[i], on_batch=lambda i: torch.manual_seed(SEED + i))
    assert step.fallbacks == before + 2 and store.invalid_batches() == [(2, 2)] and len(store) == 5
    got = store.results()
    assert sum(r["scores_3d"].shape[0] for r in got) > 0 and all(r["scores_3d"].shape[0] > 0 for r in got[2:4])
    for s, (g, w) in enumerate(zip(got, want)):
        for k in ("boxes_3d", "scores_3d", "labels_3d"):
            assert torch.equal(g[k], w[k]), (s, k)
    e1, e2 = IndoorEvaluator(world.num_classes, device=cuda), IndoorEvaluator(world.num_classes, device=cuda)
    e1.add_store(store, gts, labs)
    e2.add(want, gts, labs)
    m1, m2 = e1.compute(), e2.compute()
    assert set(m1) == set(m2) and all(np.float64(m1[k]).tobytes() == np.float64(m2[k]).tobytes() for k in m2)
    with pytest.raises(ValueError, match="tta_max_num"):
        testing.test_dataset(step, iter(batches[:1]), DetStore(5, 100, 7, cuda))
