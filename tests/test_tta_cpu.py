"""Test-time augmentation, host side: the NumPy restatement (tests/tta_ref.py) against the reference's own merge_all_aug_bboxes_3d and
bbox3d_mapping_back (projects/mmdet3d_plugin/core/merge_all_augs.py, core/bbox/util.py; loaded from where they lie with the restated
upstream helpers injected as stub modules, skipped where the reference tree is absent), the restated map-back as the inverse of the
data path's forward transforms, and the view enumeration of the TTA pipeline wrappers."""
import importlib.util
import itertools
import os
import sys
import types

import numpy as np
import pytest
import torch

import tta_ref as R
from oracle import datapath as od
from oracle import refshim

REF_CORE = os.path.join(refshim.REF_ROOT, "projects", "mmdet3d_plugin", "core")


def _load_reference(monkeypatch, box_cls):
    mods = {n: types.ModuleType(n) for n in ("mmdet3d", "mmdet3d.core", "mmdet3d.core.bbox", "mmdet3d.core.post_processing",
                                              "_ref_core", "_ref_core.bbox")}
    mods["mmdet3d"].__version__ = "1.0.0rc5"
    bb = mods["mmdet3d.core.bbox"]
    bb.bbox3d2result, bb.xywhr2xyxyr = R.torch_bbox3d2result, R.torch_xywhr2xyxyr
    bb.LiDARInstance3DBoxes = bb.DepthInstance3DBoxes = box_cls
    pp = mods["mmdet3d.core.post_processing"]
    pp.nms_bev = pp.nms_normal_bev = R.torch_nms_bev
    mods["_ref_core"].__path__ = [REF_CORE]
    mods["_ref_core.bbox"].__path__ = [os.path.join(REF_CORE, "bbox")]
    for n, m in mods.items():
        monkeypatch.setitem(sys.modules, n, m)
    out = {}
    for name, path in (("_ref_core.bbox.util", os.path.join(REF_CORE, "bbox", "util.py")),
                       ("_ref_core.merge_all_augs", os.path.join(REF_CORE, "merge_all_augs.py"))):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        monkeypatch.setitem(sys.modules, name, mod)
        spec.loader.exec_module(mod)
        out[name.rsplit(".", 1)[1]] = mod
    return out


def random_views(rng, params, coord, dim=7, n=(3, 12), ncls=3, thr=0.1, extent=8.0, size=(1.0, 4.0)):
    """one sample's per-view detections, distinct scores, every same-class IoU at least 1e-3 away from thr"""
    while True:
        views = []
        for _ in params:
            k = int(rng.integers(n[0], n[1] + 1))
            b = np.concatenate([rng.uniform(-extent, extent, (k, 2)), rng.uniform(-2, 0, (k, 1)), rng.uniform(size[0], size[1], (k, 3)),
                                rng.uniform(-np.pi, np.pi, (k, 1))] + ([rng.uniform(-3, 3, (k, 2))] if dim == 9 else []), 1).astype(np.float32)
            views.append([b, None, rng.integers(0, ncls, k)])
        tot = sum(len(v[0]) for v in views)
        sc = rng.permutation(tot).astype(np.float32) / tot + np.float32(0.01)
        o = 0
        for v in views:
            v[1] = sc[o:o + len(v[0])]
            o += len(v[0])
        ious = R.same_class_ious(views, params, coord)
        if not len(ious) or np.abs(ious - thr).min() >= 1e-3:
            return [tuple(v) for v in views]


DOUBLE_FLIP = [(0.0, 1.0, False, False), (0.0, 1.0, False, True), (0.0, 1.0, True, False), (0.0, 1.0, True, True)]


@pytest.mark.skipif(not refshim.available(), reason="reference tree absent")
@pytest.mark.parametrize("coord,dim,seed", [(R.LIDAR, 7, 0), (R.LIDAR, 9, 1), (R.DEPTH, 7, 2), (R.LIDAR, 7, 3)])
def test_restatement_matches_reference_merge(monkeypatch, coord, dim, seed):
    box_cls = R.LiDARBoxes if coord == R.LIDAR else R.DepthBoxes
    ref = _load_reference(monkeypatch, box_cls)
    rng = np.random.default_rng(seed)
    params = DOUBLE_FLIP if seed != 3 else [(0.3, 1.05, False, False), (-0.2, 0.95, True, False), (0.0, 1.0, False, True)]
    views = random_views(rng, params, coord, dim=dim)
    # bbox3d_mapping_back: the reference's own against the restatement
    for (b, _, _), (rot, sc, fh, fv) in zip(views, params):
        got = ref["util"].bbox3d_mapping_back(box_cls(torch.from_numpy(b)), rot, sc, fh, fv).tensor.numpy()
        np.testing.assert_array_equal(got, R.mapping_back(b, rot, sc, fh, fv, coord))
    aug = [dict(boxes_3d=box_cls(torch.from_numpy(b)), scores_3d=torch.from_numpy(s), labels_3d=torch.from_numpy(l)) for b, s, l in views]
    metas = [[dict(pcd_scale_factor=sc, rot_degree=rot, pcd_horizontal_flip=fh, pcd_vertical_flip=fv)] for rot, sc, fh, fv in params]
    res = ref["merge_all_augs"].merge_all_aug_bboxes_3d(aug, metas, None)
    mb, ms, ml = R.merge(views, params, coord)
    np.testing.assert_array_equal(res["labels_3d"].numpy(), ml)
    np.testing.assert_array_equal(res["scores_3d"].numpy(), ms)
    np.testing.assert_array_equal(res["boxes_3d"].tensor.numpy(), mb)
    assert 0 < len(ml) < sum(len(v[2]) for v in views)          # the NMS did something


@pytest.mark.parametrize("coord", [od.DEPTH, od.LIDAR])
@pytest.mark.parametrize("dim", [7, 9])
def test_mapping_back_inverts_the_forward_view(coord, dim):
    """a view is GlobalRotScaleTrans (rotate, scale) followed by RandomFlip3D; the restated map-back undoes it"""
    rng = np.random.default_rng(7 + dim + coord)
    b = np.concatenate([rng.uniform(-30, 30, (20, 3)), rng.uniform(0.5, 4, (20, 3)), rng.uniform(-np.pi, np.pi, (20, 1))]
                       + ([rng.uniform(-5, 5, (20, 2))] if dim == 9 else []), 1).astype(np.float32)
    for rot, sc, fh, fv in itertools.product([0.0, 0.7, -2.5], [1.0, 0.9, 1.1], [False, True], [False, True]):
        fwd = od.augment_boxes(od.augment_boxes(b, False, False, rot, sc, coord), fh, fv, 0.0, 1.0, coord)
        back = R.mapping_back(fwd, rot, sc, fh, fv, coord)
        cols = [c for c in range(dim) if c != 6]
        np.testing.assert_allclose(back[:, cols], b[:, cols], rtol=1e-5, atol=1e-5 * 30)
        assert R.yaw_close(back[:, 6], b[:, 6], 1e-5).all()


def _tta_pipeline(kind="MultiScaleFlipAug3D", **kw):
    inner = [dict(type="GlobalRotScaleTrans", rot_range=[0, 0], scale_ratio_range=[1.0, 1.0], translation_std=[0, 0, 0]),
             dict(type="RandomFlip3D"),
             dict(type="PointsRangeFilter", point_cloud_range=[0, -40, -3, 70.4, 40, 1]),
             dict(type="DefaultFormatBundle3D", class_names=["Car"], with_label=False),
             dict(type="Collect3D", keys=["points"])]
    return [dict(type="LoadPointsFromFile", coord_type="LIDAR", load_dim=4, use_dim=4),
            dict(type=kind, img_scale=(1333, 800), transforms=inner, **kw)]


def test_double_flip_pipeline_builds_and_enumerates_views_in_reference_order():
    from uni3detr_amd.datapath import DevicePipeline, MultiScaleFlipAug3D
    pipe = DevicePipeline(_tta_pipeline(pts_scale_ratio=1, flip=True, pcd_horizontal_flip=True, pcd_vertical_flip=True))
    assert pipe.skipped == ["LoadPointsFromFile"]
    (tta,) = pipe.transforms
    assert isinstance(tta, MultiScaleFlipAug3D)
    assert [(h, v) for _, _, _, h, v in tta.views()] == [(False, False), (False, True), (True, False), (True, True)]
    assert [type(t).__name__ for t in tta.inner.transforms] == ["GlobalRotScaleTrans", "RandomFlip3D", "PointsRangeFilter"]
    # flip without the per-axis switches: one flipped view, nothing mirrored (the reference's flip_aug = [True])
    single = DevicePipeline(_tta_pipeline(flip=True)).transforms[0]
    assert single.views() == [(0.0, 1.0, True, False, False)]


def test_rotation_scale_flip_views_count_and_order():
    from uni3detr_amd.datapath import DevicePipeline, MultiRotScaleFlipAug3D
    rots, scales = [0.0, 0.5, -0.5], [0.95, 1.05]
    tta = DevicePipeline(_tta_pipeline("MultiRotScaleFlipAug3D", pts_scale_ratio=scales, rotate_degree=rots, flip=True,
                                       pcd_horizontal_flip=True, pcd_vertical_flip=False)).transforms[0]
    assert isinstance(tta, MultiRotScaleFlipAug3D)
    views = tta.views()
    assert len(views) == 3 * 2 * 2
    assert views == [(r, s, True, h, False) for r in rots for s in scales for h in (False, True)]
    assert DevicePipeline(_tta_pipeline(pts_scale_ratio=[1.0, 1.1], flip=True, pcd_vertical_flip=True)).transforms[0].views() == \
        [(0.0, 1.0, True, False, False), (0.0, 1.0, True, False, True), (0.0, 1.1, True, False, False), (0.0, 1.1, True, False, True)]


def test_rotated_views_need_rotation_before_flip():
    from uni3detr_amd.datapath import MultiRotScaleFlipAug3D
    inner = [dict(type="RandomFlip3D"), dict(type="GlobalRotScaleTrans", rot_range=[0, 0], scale_ratio_range=[1.0, 1.0])]
    with pytest.raises(NotImplementedError):
        MultiRotScaleFlipAug3D(inner, pts_scale_ratio=1, rotate_degree=[0.0, 0.5], flip=True, pcd_horizontal_flip=True)


def test_merge_restatement_rules():
    """declared rules of the restatement: NaN scores dropped, label gaps skipped, stable ties, max_num cut"""
    b = np.array([[0, 0, 0, 2, 2, 1, 0], [0.1, 0, 0, 2, 2, 1, 0], [10, 0, 0, 2, 2, 1, 0], [20, 0, 0, 2, 2, 1, 0]], np.float32)
    s = np.array([0.5, 0.5, np.nan, 0.5], np.float32)
    l = np.array([4, 4, 0, 1])
    mb, ms, ml = R.merge([(b, s, l)], [(0.0, 1.0, False, False)], R.LIDAR)
    assert ml.tolist() == [1, 4] and mb[:, 0].tolist() == [20.0, 0.0]       # class-major then stable by score: class 1 first
    mb, ms, ml = R.merge([(b, s, l)], [(0.0, 1.0, False, False)], R.LIDAR, max_num=1)
    assert ml.tolist() == [1]
