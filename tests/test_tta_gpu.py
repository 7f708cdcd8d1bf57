"""GPU: test-time augmentation - the view expansion against running each view alone, the fused map-back against u3d_boxes_augment,
the device merge (csrc/tta.hip) against the NumPy restatement (tests/tta_ref.py) and against u3d_nms3d, and Uni3DETR.aug_test end to
end on small KITTI / nuScenes models."""
import ast
import os

import numpy as np
import pytest
import torch

import tta_ref as R
from test_tta_cpu import random_views
from uni3detr_amd import datapath as dp
from uni3detr_amd import native as nv
from uni3detr_amd import tta

pytestmark = pytest.mark.gpu
DOUBLE_FLIP = [(0.0, 1.0, False, False), (0.0, 1.0, False, True), (0.0, 1.0, True, False), (0.0, 1.0, True, True)]


def _metas(params):
    return [dict(rot_degree=r, pcd_scale_factor=s, pcd_horizontal_flip=h, pcd_vertical_flip=v) for r, s, h, v in params]


def _merge_scenes(cuda, scenes, params, coord, ncls, **kw):
    """scenes: per scene a list of per-view (boxes, scores, labels) numpy -> merge_aug_batch output (host numpy per scene)"""
    dets = [tuple(torch.from_numpy(np.asarray(x)).to(cuda) for x in v) for sc in scenes for v in sc]
    tab = tta.view_params(_metas(params) * len(scenes), cuda)
    res = tta.merge_aug_batch(dets, tab, len(params), coord, ncls, **kw)
    return [(r["boxes_3d"].cpu().numpy(), r["scores_3d"].cpu().numpy(), r["labels_3d"].cpu().numpy()) for r in res]


def _assert_same(got, ref, extent=30.0):
    gb, gs, gl = got
    rb, rs, rl = ref
    np.testing.assert_array_equal(gl, rl)
    np.testing.assert_allclose(gs, rs, rtol=1e-6)
    cols = [c for c in range(rb.shape[1]) if c != 6]
    np.testing.assert_allclose(gb[:, cols], rb[:, cols], rtol=1e-6, atol=1e-6 * extent)
    assert R.yaw_close(gb[:, 6], rb[:, 6], 1e-5).all()


# ---- expansion -------------------------------------------------------------------------------------------------------------------
def test_expansion_equals_each_view_alone(cuda):
    rng = np.random.default_rng(0)
    scenes = [np.concatenate([rng.uniform(-5, 75, (n, 1)), rng.uniform(-45, 45, (n, 1)), rng.uniform(-4, 2, (n, 1)), rng.uniform(0, 1, (n, 1))],
                             1).astype(np.float32) for n in (3000, 2100)]
    rng_cfg = [0, -40, -3, 70.4, 40, 1]
    inner = [dict(type="GlobalRotScaleTrans", rot_range=[0, 0], scale_ratio_range=[1.0, 1.0], translation_std=[0, 0, 0]),
             dict(type="RandomFlip3D"), dict(type="PointsRangeFilter", point_cloud_range=rng_cfg)]
    pipe = dp.DevicePipeline([dict(type="MultiRotScaleFlipAug3D", img_scale=(1333, 800), pts_scale_ratio=[1.0, 1.1], rotate_degree=[0.0, 0.4],
                                   flip=True, pcd_horizontal_flip=True, pcd_vertical_flip=True, transforms=inner)])
    views = pipe.transforms[0].views()
    A = len(views)
    assert A == 16
    batch = pipe(dp.pack_batch([torch.from_numpy(p).to(cuda) for p in scenes], box_type_3d="LiDAR"))
    assert batch["tta_views"] == A and tuple(batch["tta_params"].shape) == (2 * A, 9)
    off, cnt = batch["scene_off"].tolist(), batch["count"].tolist()
    for b, p in enumerate(scenes):
        for a, (rot, sc, _, h, v) in enumerate(views):
            one = dp.pack_batch([torch.from_numpy(p).to(cuda)], box_type_3d="LiDAR")
            one.update(rot_degree=np.array([rot], np.float32), pcd_scale_factor=np.array([sc], np.float32),
                       pcd_horizontal_flip=np.array([h]), pcd_vertical_flip=np.array([v]))
            one = dp.DevicePipeline(inner)(one)
            k = b * A + a
            got = batch["points"][off[k]:off[k] + cnt[k]]
            assert torch.equal(got, one["points"][:int(one["count"][0])]), (b, a)
            ref_tab = dp._params(dict(scene_off=one["scene_off"], points=one["points"], pcd_horizontal_flip=[h], pcd_vertical_flip=[v],
                                      pcd_rotation_angle=[rot], pcd_scale_factor=[sc]))
            assert torch.equal(batch["tta_params"][k], ref_tab[0])
    points, metas = dp.tta_forward_inputs(batch)
    assert len(points) == A and len(points[0]) == 2 and metas[3][1]["pcd_vertical_flip"] and metas[3][1]["box_type_3d"] == "LiDAR"
    assert torch.equal(points[5][1], batch["points"][off[A + 5]:off[A + 5] + cnt[A + 5]])


# ---- map-back ----------------------------------------------------------------------------------------------------------------------
def _boxes(rng, n, dim):
    return np.concatenate([rng.uniform(-30, 30, (n, 2)), rng.uniform(-2, 1, (n, 1)), rng.uniform(0.5, 4, (n, 3)), rng.uniform(-3, 3, (n, 1))]
                          + ([rng.uniform(-5, 5, (n, 2))] if dim == 9 else []), 1).astype(np.float32)


@pytest.mark.parametrize("coord", [R.DEPTH, R.LIDAR])
@pytest.mark.parametrize("dim", [7, 9])
def test_map_back_is_bit_identical_to_boxes_augment_and_inverts_the_view(cuda, coord, dim):
    rng = np.random.default_rng(dim + 10 * coord)
    params = [(r, s, h, v) for r in (0.0, 0.6, -1.9) for s in (1.0, 0.93) for h in (False, True) for v in (False, True)]
    V, n = len(params), 25
    raw = torch.from_numpy(_boxes(rng, V * n, dim)).to(cuda)
    scores = torch.from_numpy(rng.permutation(V * n).astype(np.float32) / (V * n) + 0.01).to(cuda)
    labels = torch.zeros(V * n, dtype=torch.int32, device=cuda)
    tab = tta.view_params(_metas(params), cuda)
    off = list(range(0, V * n + 1, n))
    # nms_thr 2: nothing is suppressed, the output is every mapped-back candidate by descending score
    ob, os_, ol, oc = nv.tta_merge(raw, scores, labels, off, tab, V, coord, 1, nms_thr=2.0, max_num=V * n)
    assert int(oc[0]) == V * n
    order = torch.argsort(scores, descending=True, stable=True)
    ref = raw.clone()
    nv.boxes_augment(ref, torch.tensor(off, dtype=torch.int32, device=cuda), nv.tta_inverse_params(tab), coord)
    diff = (ob[0] != ref[order]).nonzero()
    assert diff.numel() == 0, ("rows, columns differing:", diff[:8].tolist())
    assert torch.equal(os_[0], scores[order])
    # round trip: the view's forward (rotate + scale, then flip) followed by the map-back returns the originals
    off_d = torch.tensor(off, dtype=torch.int32, device=cuda)
    rs = tab.clone()
    rs[:, 0:2] = 0
    fl = torch.zeros_like(tab)
    fl[:, 0:2], fl[:, 3], fl[:, 5] = tab[:, 0:2], 1.0, 1.0
    fwd = raw.clone()
    nv.boxes_augment(fwd, off_d, rs, coord)
    nv.boxes_augment(fwd, off_d, fl, coord)
    ob, _, _, _ = nv.tta_merge(fwd, scores, labels, off, tab, V, coord, 1, nms_thr=2.0, max_num=V * n)
    got, want = ob[0].cpu().numpy(), raw[order].cpu().numpy()
    cols = [c for c in range(dim) if c != 6]
    np.testing.assert_allclose(got[:, cols], want[:, cols], rtol=1e-5, atol=1e-5 * 30)
    assert R.yaw_close(got[:, 6], want[:, 6], 1e-5).all()


# ---- merge against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coord,dim", [(R.LIDAR, 7), (R.LIDAR, 9), (R.DEPTH, 7)])
def test_merge_matches_restatement_on_random_scenes(cuda, coord, dim):
    rng = np.random.default_rng(3 + dim + coord)
    params = [(0.2, 1.05, False, False), (0.2, 1.05, True, True), (-0.3, 0.95, False, True), (0.0, 1.0, True, False)]
    scenes = [random_views(rng, params, coord, dim=dim, n=(5, 30), ncls=4) for _ in range(3)]
    got = _merge_scenes(cuda, scenes, params, coord, 4)
    for g, sc in zip(got, scenes):
        _assert_same(g, R.merge(sc, params, coord))
    # B scenes at once == each scene alone
    for b, sc in enumerate(scenes):
        (alone,) = _merge_scenes(cuda, [sc], params, coord, 4)
        for x, y in zip(alone, got[b]):
            np.testing.assert_array_equal(x, y)


def test_merge_edge_cases(cuda):
    rng = np.random.default_rng(11)
    P = DOUBLE_FLIP
    empty = [(np.zeros((0, 7), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32)) for _ in P]
    single = random_views(rng, P, R.LIDAR, ncls=1)
    # all candidates suppressed by the first: the same box in every view (mapped back), descending scores
    box = np.array([[10.0, 5.0, -1.0, 4.0, 2.0, 1.5, 0.3]], np.float32)
    dup = []
    for k, (_, _, h, v) in enumerate(P):
        t = R.flip_boxes(box, "horizontal", R.LIDAR) if h else box
        t = R.flip_boxes(t, "vertical", R.LIDAR) if v else t
        dup.append((np.repeat(t, 3, 0), np.array([0.9, 0.8, 0.7], np.float32) - 0.01 * k, np.full(3, 2, np.int32)))
    # label gaps and NaN scores
    gaps = [(b, s.copy(), (l * 3).astype(np.int32)) for b, s, l in random_views(rng, P, R.LIDAR, ncls=3)]
    gaps[1][1][0] = np.nan
    gaps[2][1][-1] = np.inf
    scenes = [empty, single, dup, gaps, empty]
    got = _merge_scenes(cuda, scenes, P, R.LIDAR, 7)
    for g, sc in zip(got, scenes):
        _assert_same(g, R.merge(sc, P, R.LIDAR))
    assert len(got[0][2]) == 0 and len(got[4][2]) == 0 and len(got[2][2]) == 1
    assert np.isfinite(got[3][1]).all()
    # more than max_num survivors
    got = _merge_scenes(cuda, [single, gaps], P, R.LIDAR, 7, max_num=5)
    for g, sc in zip(got, [single, gaps]):
        _assert_same(g, R.merge(sc, P, R.LIDAR, max_num=5))
        assert len(g[2]) == 5
    # scenes without a detection in front of, between and behind the others
    scenes = [empty, single, empty, gaps, empty]
    for g, sc in zip(_merge_scenes(cuda, scenes, P, R.LIDAR, 7), scenes):
        _assert_same(g, R.merge(sc, P, R.LIDAR))


def test_merge_large_segment_takes_the_global_path(cuda):
    """one class with more candidates than the LDS path holds: a grid of unit squares, every second one duplicated 0.2 m off
    (IoU 2/3: suppressed), plus a second, small class served by the LDS path in the same call"""
    rng = np.random.default_rng(5)
    g = np.stack(np.meshgrid(np.arange(46), np.arange(46)), -1).reshape(-1, 2).astype(np.float32) * 1.5
    base = np.concatenate([g, np.zeros((len(g), 1)), np.ones((len(g), 3)), np.zeros((len(g), 1))], 1).astype(np.float32)
    shifted = base[::2].copy()
    shifted[:, 0] += 0.2
    big = np.concatenate([base, shifted])
    n = len(big)
    assert n > nv.TTA_LDS_CAP
    small = base[:40].copy()
    small[:, 1] += 0.1
    boxes = np.concatenate([big, small])
    labels = np.concatenate([np.zeros(n, np.int32), np.ones(40, np.int32)])
    scores = (rng.permutation(len(boxes)).astype(np.float32) + 1) / len(boxes)
    half = len(boxes) // 2
    views = [(boxes[:half], scores[:half], labels[:half]), (boxes[half:], scores[half:], labels[half:])]
    P = [(0.0, 1.0, False, False), (0.0, 1.0, False, False)]
    (got,) = _merge_scenes(cuda, [views], P, R.LIDAR, 2, max_num=5000)
    ref = R.merge(views, P, R.LIDAR, max_num=5000)
    _assert_same(got, ref, extent=70.0)
    assert len(got[2]) < n


def test_merge_equals_nms3d_classwise_on_dyadic_boxes(cuda):
    rng = np.random.default_rng(21)
    while True:
        n = 300
        b = np.concatenate([rng.integers(-64, 64, (n, 2)) / 8.0, rng.uniform(-2, 0, (n, 1)), rng.integers(4, 16, (n, 2)) / 4.0,
                            rng.uniform(1, 2, (n, 1)), rng.uniform(-3, 3, (n, 1))], 1).astype(np.float32)
        s = (rng.permutation(n).astype(np.float32) + 1) / n
        l = rng.integers(0, 3, n).astype(np.int32)
        views = [(b, s, l)]
        ious = R.same_class_ious(views, [(0.0, 1.0, False, False)], R.LIDAR)
        if np.abs(ious - 0.1).min() >= 1e-3:
            break
    (got,) = _merge_scenes(cuda, [views], [(0.0, 1.0, False, False)], R.LIDAR, 3)
    bt, st, lt = (torch.from_numpy(x).to(cuda) for x in (b, s, l))
    keep = nv.nms3d_classwise(bt, st, lt.long(), 0.1)
    keep = keep[torch.argsort(st[keep], descending=True, stable=True)][:500]
    assert np.array_equal(got[0], b[keep.cpu().numpy()]) and np.array_equal(got[1], s[keep.cpu().numpy()])
    assert np.array_equal(got[2], l[keep.cpu().numpy()])
    assert len(got[2]) < n


# ---- end to end --------------------------------------------------------------------------------------------------------------------
SHIPPED = os.path.join(os.path.dirname(__file__), "golden", "shipped_configs.txt")


@pytest.mark.parametrize("name,npts", [("kitti_3classes", 16000), ("nuscenes", 30000)])
def test_aug_test_end_to_end(cuda, name, npts, monkeypatch):
    from uni3detr_amd.evaluation import IndoorEvaluator
    from uni3detr_amd.registry import build_model, to_config
    from uni3detr_amd.synth import room_scene
    cfg = to_config(ast.literal_eval(open(SHIPPED).read())[name]["config"]["model"])
    model = build_model(cfg).to(cuda).eval()
    pc = tuple(cfg["pts_voxel_layer"]["point_cloud_range"])
    nfeat = cfg["pts_middle_encoder"]["in_channels"]
    B = 2
    raw = []
    for i in range(B):
        p = room_scene(i, npts - 1000 * i, pc_range=pc)[0]
        if nfeat > 4:
            p = np.concatenate([p, np.zeros((p.shape[0], nfeat - 4), np.float32)], 1)
        raw.append(torch.from_numpy(p).to(cuda))
    inner = [dict(type="GlobalRotScaleTrans", rot_range=[0, 0], scale_ratio_range=[1.0, 1.0], translation_std=[0, 0, 0]),
             dict(type="RandomFlip3D"), dict(type="PointsRangeFilter", point_cloud_range=list(pc))]
    pipe = dp.DevicePipeline([dict(type="MultiScaleFlipAug3D", img_scale=(1333, 800), pts_scale_ratio=1, flip=True, pcd_horizontal_flip=True,
                                   pcd_vertical_flip=True, transforms=inner)])
    batch = pipe(dp.pack_batch(raw, box_type_3d="LiDAR"))
    points, metas = dp.tta_forward_inputs(batch)
    A = len(points)
    assert A == 4
    calls, seen = [], []
    orig = model.extract_pts_feat
    monkeypatch.setattr(model, "extract_pts_feat", lambda pts: calls.append(len(pts)) or orig(pts))
    orig_bb = model.pts_bbox_head.get_bboxes

    def record(*a, **k):
        out = orig_bb(*a, **k)
        seen.extend([(bx.cpu().numpy(), sc.cpu().numpy(), lb.cpu().numpy()) for bx, sc, lb in out])
        return out
    monkeypatch.setattr(model.pts_bbox_head, "get_bboxes", record)
    res = model(return_loss=False, img_metas=metas, points=points)
    assert calls == [B * A]                                              # one batched forward for every view of every sample
    assert len(res) == B and len(seen) == B * A
    flat_m = [metas[a][b] for b in range(B) for a in range(A)]
    params = [(m["rot_degree"], m["pcd_scale_factor"], m["pcd_horizontal_flip"], m["pcd_vertical_flip"]) for m in flat_m[:A]]
    ncls = cfg["pts_bbox_head"]["num_classes"]
    tab = tta.view_params(flat_m[:A], cuda)
    for b in range(B):
        # the detections get_bboxes gave for this sample's views (the B*A batch simple_test would run), merged on the host
        views = seen[b * A:(b + 1) * A]
        ref = R.merge(views, params, R.LIDAR)
        got = (res[b]["boxes_3d"].numpy(), res[b]["scores_3d"].numpy(), res[b]["labels_3d"].numpy())
        assert set(res[b]) == {"boxes_3d", "scores_3d", "labels_3d"} and len(ref[2]) > 0
        ious = R.same_class_ious(views, params, R.LIDAR)
        if len(ious) == 0 or np.abs(ious - 0.1).min() >= 1e-4:
            _assert_same(got, ref, extent=100.0)
        else:                                                            # a pair at the threshold: f32 vs float64 IoU may differ there
            assert abs(len(got[2]) - len(ref[2])) <= 2
        # the batched merge of all samples == this sample's detections merged alone
        dets = [tuple(torch.from_numpy(x).to(cuda) for x in v) for v in views]
        (alone,) = tta.merge_aug_batch(dets, tab, A, tta.LIDAR, ncls)
        for k in alone:
            assert torch.equal(alone[k].cpu(), res[b][k]), (b, k)
    # simple_test on the same expanded batch serves the same views (shapes; the forward itself is not bitwise reproducible)
    single = model.simple_test(flat_m, [points[a][b] for b in range(B) for a in range(A)])
    assert len(single) == B * A and all(r["boxes_3d"].shape[1] == seen[0][0].shape[1] for r in single)
    # chunks of whole samples (one sample per forward): the same scenes, merged the same way
    resc = model.aug_test(points, metas, max_batch=A)
    assert len(resc) == B
    ev = IndoorEvaluator(cfg["pts_bbox_head"]["num_classes"], device=cuda)
    gt = [res[b]["boxes_3d"][:3].clone() for b in range(B)]
    ev.add(res, [g[:, :7] for g in gt], [res[b]["labels_3d"][:3] for b in range(B)])
    assert len(ev) == B
