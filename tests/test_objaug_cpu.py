"""GT-paste / ObjectNoise host side: the NumPy restatement (tests/objaug_ref.py) and the product's database + draws
(uni3detr_amd/gtdb.py, datapath.ObjectSample.draw) against the reference's own UnifiedDataBaseSampler and UnifiedObjectSample
(projects/mmdet3d_plugin/datasets/pipelines/dbsampler.py, transform_3d.py:591-786; loaded from where they lie with the restated
upstream helpers injected as stub modules, skipped where the reference tree is absent), and property checks of the restatement."""
import importlib.util
import math
import os
import pickle
import sys
import types

import numpy as np
import pytest
import torch

import objaug_ref as R
from oracle import boxes as ob
from oracle.refshim import REF_ROOT

REF_PIPE = os.path.join(REF_ROOT, "projects", "mmdet3d_plugin", "datasets", "pipelines")
CLASSES = ["Car", "Pedestrian", "Cyclist"]


class _A:
    """.numpy() of a host array (what the reference calls on tensors)."""

    def __init__(self, a):
        self.a = a

    def numpy(self):
        return self.a


class _Points:
    """Stand-in for mmdet3d LiDARPoints: what UnifiedObjectSample / sample_all touch."""

    def __init__(self, a):
        self.a = np.asarray(a, np.float64)

    coord = property(lambda self: _A(self.a[:, :3]))
    tensor = property(lambda self: _A(self.a))

    def translate(self, t):
        self.a[:, :3] += np.asarray(t)[:3]

    def cat(self, lst):
        return _Points(np.concatenate([p.a for p in lst]))

    def __len__(self):
        return len(self.a)

    def __getitem__(self, m):
        return _Points(self.a[m])


class _Boxes:
    def __init__(self, a):
        self.tensor = _A(np.asarray(a, np.float64))

    def new_box(self, a):
        return _Boxes(a)


class _Registry:
    def __init__(self):
        self.m = {}

    def register_module(self, name=None, module=None, force=False):
        def deco(cls):
            self.m[name or cls.__name__] = cls
            return cls
        return deco


def _build_from_cfg(cfg, reg):
    cfg = dict(cfg)
    return reg.m[cfg.pop("type")](**cfg)


def _load_reference(monkeypatch, files):
    if not os.path.exists(os.path.join(REF_PIPE, "dbsampler.py")):
        pytest.skip("reference tree not available")
    for name, t in (("int", int), ("long", np.int64), ("bool", np.bool_)):       # removed from NumPy 2; the reference still names them
        monkeypatch.setattr(np, name, t, raising=False)
    PIPELINES, OBJECTSAMPLERS = _Registry(), _Registry()

    @PIPELINES.register_module()
    class LoadPointsFromFile:
        def __init__(self, coord_type="LIDAR", load_dim=4, use_dim=(0, 1, 2, 3), **kw):
            self.load_dim, self.use_dim = load_dim, list(range(use_dim)) if isinstance(use_dim, int) else list(use_dim)

        def __call__(self, results):
            p = np.fromfile(results["pts_filename"], dtype=np.float32).reshape(-1, self.load_dim)[:, self.use_dim]
            return dict(points=_Points(p))

    mods = {n: types.ModuleType(n) for n in ("mmcv", "mmcv.utils", "cv2", "mmdet3d", "mmdet3d.core", "mmdet3d.core.bbox",
                                              "mmdet3d.core.bbox.box_np_ops", "mmdet3d.datasets", "mmdet3d.datasets.builder",
                                              "mmdet3d.datasets.pipelines", "mmdet3d.datasets.pipelines.data_augment_utils",
                                              "mmdet3d.datasets.pipelines.dbsampler", "mmdet3d.utils")}
    mods["mmcv"].load = lambda p: pickle.load(open(p, "rb"))
    mods["mmcv"].build_from_cfg = mods["mmcv.utils"].build_from_cfg = _build_from_cfg
    mods["mmcv"].utils = mods["mmcv.utils"]
    mods["mmdet3d"].__version__ = "1.0.0rc5"
    bnp = mods["mmdet3d.core.bbox.box_np_ops"]
    bnp.center_to_corner_box2d, bnp.points_in_rbbox = R.center_to_corner_box2d, R.points_in_rbbox
    bb = mods["mmdet3d.core.bbox"]
    bb.box_np_ops, bb.CameraInstance3DBoxes, bb.DepthInstance3DBoxes, bb.LiDARInstance3DBoxes = bnp, object, object, _Boxes
    mods["mmdet3d.datasets.pipelines.data_augment_utils"].box_collision_test = R.box_collision_test
    mods["mmdet3d.datasets.pipelines.dbsampler"].BatchSampler = R.BatchSampler
    mods["mmdet3d.datasets.pipelines"].data_augment_utils = mods["mmdet3d.datasets.pipelines.data_augment_utils"]
    mods["mmdet3d.datasets"].PIPELINES = mods["mmdet3d.datasets.builder"].PIPELINES = PIPELINES
    mods["mmdet3d.datasets.builder"].OBJECTSAMPLERS = OBJECTSAMPLERS
    mods["mmdet3d.utils"].get_root_logger = lambda: types.SimpleNamespace(info=lambda *a, **k: None)
    for n, m in mods.items():
        monkeypatch.setitem(sys.modules, n, m)
    out = {}
    for f in ("dbsampler", "transform_3d"):
        spec = importlib.util.spec_from_file_location(f"_ref_{f}", os.path.join(REF_PIPE, f + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        out[f] = mod
    return out


def _synthetic_db(tmp_path, rng):
    """A KITTI-shaped *_dbinfos_train.pkl + .bin files: three classes and a key outside them, difficulties -1..2, a few objects with
    too few points (filter_by_min_points)."""
    infos, sizes = {}, dict(Car=(3.9, 1.6, 1.5), Pedestrian=(0.8, 0.6, 1.7), Cyclist=(1.8, 0.6, 1.7), Van=(5.0, 2.0, 2.2))
    for key, n in (("Pedestrian", 9), ("Car", 23), ("Van", 4), ("Cyclist", 7)):
        infos[key] = []
        for i in range(n):
            dx, dy, dz = sizes[key]
            box = np.array([rng.uniform(5, 60), rng.uniform(-30, 30), rng.uniform(-2, -1), dx, dy, dz, rng.uniform(-np.pi, np.pi)],
                           np.float32)
            m = int(rng.integers(2, 40))
            local = np.stack([rng.uniform(-0.45, 0.45, m) * dx, rng.uniform(-0.45, 0.45, m) * dy, rng.uniform(0.05, 0.95, m) * dz], 1)
            c, s = np.cos(box[6]), np.sin(box[6])
            p = np.stack([local[:, 0] * c - local[:, 1] * s, local[:, 0] * s + local[:, 1] * c, local[:, 2], rng.uniform(0, 1, m)], 1)
            path = f"{key}_{i}.bin"
            p.astype(np.float32).tofile(str(tmp_path / path))
            infos[key].append(dict(name=key, path=path, box3d_lidar=box, num_points_in_gt=m, difficulty=int(rng.integers(-1, 3))))
    with open(tmp_path / "db.pkl", "wb") as f:
        pickle.dump(infos, f)
    return infos


def _scene(rng, n_pts, n_gt):
    p = np.stack([rng.uniform(0, 70, n_pts), rng.uniform(-40, 40, n_pts), rng.uniform(-3, 1, n_pts), rng.uniform(0, 1, n_pts)], 1)
    g = np.stack([rng.uniform(5, 60, n_gt), rng.uniform(-30, 30, n_gt), rng.uniform(-2, -1, n_gt), rng.uniform(1, 4, n_gt),
                  rng.uniform(0.6, 1.8, n_gt), rng.uniform(1.4, 1.8, n_gt), rng.uniform(-np.pi, np.pi, n_gt)], 1)
    return p, g, rng.integers(-1, 3, n_gt)


@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_and_product_draws_match_reference_object_sample(monkeypatch, tmp_path, seed):
    files = {}
    ref = _load_reference(monkeypatch, files)
    from uni3detr_amd import datapath as dp
    from uni3detr_amd.gtdb import GTDatabase
    rng = np.random.default_rng(seed)
    _synthetic_db(tmp_path, rng)
    cfg = dict(type="UnifiedDataBaseSampler", data_root=str(tmp_path), info_path=str(tmp_path / "db.pkl"), rate=1.0,
               prepare=dict(filter_by_difficulty=[-1], filter_by_min_points=dict(Car=5, Pedestrian=10, Cyclist=10)), classes=CLASSES,
               sample_groups=dict(Car=12, Pedestrian=4, Cyclist=4),
               points_loader=dict(type="LoadPointsFromFile", coord_type="LIDAR", load_dim=4, use_dim=[0, 1, 2, 3]))
    scenes = [_scene(rng, 3000, n) for n in (6, 0, 14, 3)]

    np.random.seed(100 + seed)
    tf = ref["transform_3d"].UnifiedObjectSample(db_sampler=dict(cfg))
    want = []
    for p, g, l in scenes:
        out = tf(dict(gt_bboxes_3d=_Boxes(g), gt_labels_3d=l.copy(), points=_Points(p)))
        want.append(out)

    np.random.seed(100 + seed)
    db = GTDatabase.from_infos(str(tmp_path / "db.pkl"), str(tmp_path), CLASSES, cfg["prepare"], cfg["points_loader"], device="cpu")
    t = dp.UnifiedObjectSample(db_sampler=dict(cfg), gt_database=db)
    pts_h, off_h = db.points.numpy(), db.obj_off_host
    wrapped = False
    for (p, g, l), w in zip(scenes, want):
        hist = np.array([np.sum(l == c) for c in range(len(CLASSES))])
        before = {k: s._idx for k, s in db.samplers.items()}
        rows, grp = t.draw(hist)
        wrapped |= any(db.samplers[k]._idx < before[k] for k in before)
        got = R.paste_scene(p, g, l, db.boxes_host[rows], db.labels.numpy()[rows], [pts_h[off_h[r]:off_h[r + 1]] for r in rows], grp,
                            sampled_first=False)
        assert np.array_equal(got["labels"], w["gt_labels_3d"])
        np.testing.assert_array_equal(got["boxes"], w["gt_bboxes_3d"].tensor.numpy())
        np.testing.assert_array_equal(got["points"], w["points"].a)
        if "points_idx" in w:
            np.testing.assert_array_equal(got["points_idx"], w["points_idx"])
    assert wrapped                                   # a class sampler ran out and reshuffled on the way


def test_collision_agrees_with_bev_intersection_area():
    """box_collision_test == "rotated intersection area > 0" (oracle/boxes.py, the rotated-IoU arithmetic) on random pairs kept at
    least 1e-3 away from touching."""
    rng = np.random.default_rng(11)
    n_pos = n_neg = 0
    while n_pos + n_neg < 600:
        a = np.array([0, 0, rng.uniform(0.3, 4), rng.uniform(0.3, 4), rng.uniform(-np.pi, np.pi)])
        b = np.array([rng.uniform(-4, 4), rng.uniform(-4, 4), rng.uniform(0.3, 4), rng.uniform(0.3, 4), rng.uniform(-np.pi, np.pi)])
        area = ob.rotated_intersection_area(a, b)
        ca, cb = (R.center_to_corner_box2d(x[None, :2], x[None, 2:4], x[None, 4])[0] for x in (a, b))
        if area == 0 and _gap(ca, cb) < 1e-3 or 0 < area < 1e-3:
            continue
        got = bool(R.box_collision_test(ca[None], cb[None])[0, 0])
        assert got == (area > 0), (a, b, area)
        n_pos += got
        n_neg += not got
    assert n_pos > 100 and n_neg > 100
    inner = R.center_to_corner_box2d(np.zeros((1, 2)), np.array([[0.5, 0.5]]), np.array([0.3]))
    outer = R.center_to_corner_box2d(np.zeros((1, 2)), np.array([[3.0, 2.0]]), np.array([0.0]))
    assert R.box_collision_test(inner, outer)[0, 0] and R.box_collision_test(outer, inner)[0, 0]       # containment, no edge crossing


def _gap(a, b):
    def seg(p, q, r):
        d = r - q
        t = np.clip(np.dot(p - q, d) / np.dot(d, d), 0, 1)
        return np.linalg.norm(p - (q + t * d))
    return min(min(seg(p, x[i], x[(i + 1) % 4]) for i in range(4)) for p, x in [(p, b) for p in a] + [(p, a) for p in b])


def test_batch_sampler_returns_the_tail_and_reshuffles():
    from uni3detr_amd.gtdb import BatchSampler
    np.random.seed(3)
    s = BatchSampler(5, "Car")
    np.random.seed(3)
    r = R.BatchSampler(list(range(5)), "Car")
    first = s.sample(3).copy()              # a view of the index list (upstream too): the reshuffle below reorders it
    assert list(first) == r.sample(3) and len(first) == 3
    tail = s.sample(3)                                # idx 3 + 3 >= 5: the two that are left, then a reshuffle
    assert len(tail) == 2 and list(tail) == r.sample(3) and s._idx == 0
    assert sorted(list(first) + list(tail)) == list(range(5))
    assert len(s.sample(5)) == 5 and s._idx == 0        # idx + num == n also resets


def test_greedy_rule_rejects_on_a_later_candidate_of_the_same_class():
    """sample_class_v2: A collides with B (later, same class) -> A rejected even though B is then rejected too (B collides with C,
    which comes after it); C, cleared of both, is accepted.  In a per-candidate "first come" rule A would be kept instead."""
    gt = np.zeros((0, 7))
    A = [0.0, 0, 0, 2, 1, 1, 0]
    B = [1.8, 0, 0, 2, 0.8, 1, 0]          # overlaps A and C
    C = [3.6, 0, 0, 2, 1, 1, 0]
    acc = R.greedy_accept(gt, np.array([A, B, C]), np.array([0, 0, 0]))
    assert acc.tolist() == [False, False, True]
    # the same three boxes as three classes: A first, B collides with the accepted A, C is clear of A
    assert R.greedy_accept(gt, np.array([A, B, C]), np.array([0, 1, 2])).tolist() == [True, False, True]


def test_noise_keeps_points_in_their_box_frame():
    rng = np.random.default_rng(5)
    boxes = np.array([[0, 0, 0, 2, 1, 1, 0.3], [6, 0, 0, 2, 1, 1, -0.4], [0, 6, 0, 1, 1, 2, 1.0]], np.float64)
    owner = np.repeat(np.arange(3), 20)
    local = rng.uniform(-0.4, 0.4, (60, 3)) * boxes[owner, 3:6] + np.array([0, 0, 0.5]) * boxes[owner, 3:6]
    pts = np.zeros((60, 4))
    for i, (b, q) in enumerate(zip(boxes[owner], local)):
        c, s = math.cos(b[6]), math.sin(b[6])
        pts[i, :3] = [q[0] * c - q[1] * s + b[0], q[0] * s + q[1] * c + b[1], q[2] + b[2]]
    loc = rng.normal(0, [1, 1, 0.5], (3, 20, 3))
    rot = rng.uniform(-np.pi / 4, np.pi / 4, (3, 20))
    nb, npnt, chosen = R.object_noise(boxes, pts, loc, rot)
    assert (chosen >= 0).all()
    assert R.points_in_rbbox(npnt, nb)[np.arange(60), owner].all()
