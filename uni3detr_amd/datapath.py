"""On-device training data path: the transforms of the shipped train pipelines applied to a packed batch that is
already resident in HBM, so that real-data epochs are not bound by DataLoader workers.

Mirrors the pipeline entries the configs name (ref: projects/configs/uni3detr/uni3detr_sunrgbd.py:150-174 and the plugin's
Unified* variants, projects/mmdet3d_plugin/datasets/pipelines/transform_3d.py:325-589): same `type` names, same constructor
arguments, same result-dict keys (`pcd_horizontal_flip`, `pcd_vertical_flip`, `pcd_rotation_angle`, `pcd_scale_factor`,
`uni_rot_aug`), one call for the whole BATCH instead of one per sample.  The random draws are host-side numpy draws exactly as in
the reference (`np.random.rand() < ratio`, `np.random.uniform(lo, hi)`: one per scene, in scene order, flip transforms first), the
arithmetic runs in libu3d_hip.so (uni3detr_amd/csrc/datapath.hip) - there is no host/torch fallback.

A batch is a dict: points [N,F] f32 (all scenes packed), scene_off int32 [B+1] (device), optional count int32 [B] (live rows at
the front of every scene's segment, set by PointsRangeFilter), gt_bboxes_3d [G,7|9] f32 packed + gt_off int32 [B+1] (device).
"""
import os

import numpy as np
import torch

from . import native as nv
from .registry import Registry

PIPELINES = Registry("pipeline")
OBJECT_AUG = Registry("object_aug")          # opt-in entries: built only when DevicePipeline is given what they need
DEPTH, LIDAR = 0, 1


def _coord(batch):
    return LIDAR if str(batch.get("box_type_3d", "Depth")).lower().startswith("lidar") else DEPTH


def _params(batch):
    """Device parameter table [B,9] = (flip_h, flip_v, sin, cos, angle, scale, tx, ty, tz) from the draws recorded in the batch dict."""
    B = batch["scene_off"].numel() - 1
    fh = np.asarray(batch.get("pcd_horizontal_flip", np.zeros(B, bool)), np.float32)
    fv = np.asarray(batch.get("pcd_vertical_flip", np.zeros(B, bool)), np.float32)
    ang = np.asarray(batch.get("pcd_rotation_angle", np.zeros(B)), np.float32)
    sc = np.asarray(batch.get("pcd_scale_factor", np.ones(B)), np.float32)
    tr = np.asarray(batch.get("pcd_trans", np.zeros((B, 3))), np.float32).reshape(B, 3)
    tab = np.concatenate([np.stack([fh, fv, np.sin(ang), np.cos(ang), ang, sc], 1), tr], 1).astype(np.float32)
    return torch.from_numpy(tab).to(batch["points"].device)


def _apply(batch, fh, fv, ang, sc, height_dim, trans=None):
    """One launch over the points (+ one over the boxes) for the given per-scene draws; identity entries cost nothing extra."""
    B = batch["scene_off"].numel() - 1
    tmp = dict(scene_off=batch["scene_off"], points=batch["points"], pcd_horizontal_flip=fh, pcd_vertical_flip=fv,
               pcd_rotation_angle=ang, pcd_scale_factor=sc, pcd_trans=np.zeros((B, 3), np.float32) if trans is None else trans)
    tab = _params(tmp)
    coord = _coord(batch)
    nv.points_augment(batch["points"], batch["scene_off"], tab, coord, height_dim)
    g = batch.get("gt_bboxes_3d")
    if g is not None and g.shape[0] > 0:
        nv.boxes_augment(g, batch["gt_off"], tab, coord)
    # the matrix the Unified* transforms publish (transform_3d.py:461-464, :564-567), per scene, composed with earlier transforms
    mats = []
    for b in range(B):
        s, c = np.float32(np.sin(np.float32(ang[b]))), np.float32(np.cos(np.float32(ang[b])))
        flip = np.eye(3, dtype=np.float32)
        if fh[b]:
            flip[1, 1] *= -1
        if fv[b]:
            flip[0, 0] *= -1
        m = flip @ (np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]], np.float32) @ (np.eye(3, dtype=np.float32) * np.float32(sc[b])))
        prev = batch.get("uni_rot_aug")
        mats.append(m if prev is None else prev[b] @ m)
    batch["uni_rot_aug"] = mats
    return batch


@PIPELINES.register_module()
class RandomFlip3D:
    """ref: mmdet3d RandomFlip3D as configured at uni3detr_sunrgbd.py:159-163 (sync_2d has no effect without images)."""

    def __init__(self, sync_2d=True, flip_ratio_bev_horizontal=0.0, flip_ratio_bev_vertical=0.0, **kwargs):
        assert 0 <= flip_ratio_bev_horizontal <= 1 and 0 <= flip_ratio_bev_vertical <= 1
        self.flip_ratio_bev_horizontal, self.flip_ratio_bev_vertical = flip_ratio_bev_horizontal, flip_ratio_bev_vertical

    def __call__(self, batch):
        B = batch["scene_off"].numel() - 1
        # the reference draws per sample: horizontal first, then vertical (transform_3d.py:552-559)
        if "pcd_horizontal_flip" not in batch or "pcd_vertical_flip" not in batch:
            fh, fv = np.zeros(B, bool), np.zeros(B, bool)
            for b in range(B):
                fh[b] = np.random.rand() < self.flip_ratio_bev_horizontal
                fv[b] = np.random.rand() < self.flip_ratio_bev_vertical
            batch.setdefault("pcd_horizontal_flip", fh)
            batch.setdefault("pcd_vertical_flip", fv)
        fh, fv = np.asarray(batch["pcd_horizontal_flip"], bool), np.asarray(batch["pcd_vertical_flip"], bool)
        batch.setdefault("transformation_3d_flow", []).extend(["HF"] * int(fh.any()) + ["VF"] * int(fv.any()))
        return _apply(batch, fh, fv, np.zeros(B, np.float32), np.ones(B, np.float32), -1)


@PIPELINES.register_module()
class UnifiedRandomFlip3D(RandomFlip3D):
    """ref: transform_3d.py:486-589 (same geometry; `uni_rot_aug` is published by both classes here)."""


@PIPELINES.register_module()
class GlobalRotScaleTrans:
    """ref: mmdet3d GlobalRotScaleTrans as configured at uni3detr_sunrgbd.py:164-168 and, with translation_std = [.1, .1, .1], in the
    two ScanNet configs (uni3detr_scannet.py / uni3detr_scannet_large.py train_pipeline): rotate -> scale -> translate, the translation
    one normal draw per axis and scene added to the points and to the box centres (upstream `_trans_bbox_points`, recalled)."""

    def __init__(self, rot_range=(-0.78539816, 0.78539816), scale_ratio_range=(0.95, 1.05), translation_std=(0, 0, 0), shift_height=False):
        if not isinstance(rot_range, (list, tuple, np.ndarray)):
            rot_range = [-rot_range, rot_range]
        if not isinstance(translation_std, (list, tuple, np.ndarray)):
            translation_std = [translation_std] * 3
        assert len(translation_std) == 3 and all(t >= 0 for t in translation_std), "invalid translation_std"
        self.translation_std = np.asarray(translation_std, np.float32)
        self.rot_range, self.scale_ratio_range, self.shift_height = list(rot_range), list(scale_ratio_range), shift_height

    def __call__(self, batch):
        B = batch["scene_off"].numel() - 1
        if "pcd_rotation_angle" not in batch:        # per sample: rotation first, then scale, then translation (transform_3d.py:456-460)
            ang, sc, tr = np.zeros(B, np.float32), np.ones(B, np.float32), np.zeros((B, 3), np.float32)
            preset = batch.get("rot_degree")         # a test-time view's angle (transform_3d.py:368-372)
            for b in range(B):
                ang[b] = preset[b] if preset is not None else np.random.uniform(self.rot_range[0], self.rot_range[1])
                sc[b] = np.random.uniform(self.scale_ratio_range[0], self.scale_ratio_range[1])
                if np.any(self.translation_std != 0):
                    tr[b] = np.random.normal(scale=self.translation_std, size=3)
            batch["pcd_rotation_angle"] = ang
            batch.setdefault("pcd_scale_factor", sc)
            batch.setdefault("pcd_trans", tr)
        ang = np.asarray(batch["pcd_rotation_angle"], np.float32)
        sc = np.asarray(batch.get("pcd_scale_factor", np.ones(B)), np.float32)
        tr = np.asarray(batch.get("pcd_trans", np.zeros((B, 3))), np.float32).reshape(B, 3)
        hd = int(batch.get("height_dim", 3)) if self.shift_height else -1
        batch.setdefault("transformation_3d_flow", []).extend(["R", "S", "T"])
        return _apply(batch, np.zeros(B, bool), np.zeros(B, bool), ang, sc, hd, tr)


@PIPELINES.register_module()
class UnifiedRotScaleTrans(GlobalRotScaleTrans):
    """ref: transform_3d.py:326-483."""

    def __init__(self, rot_range=(-0.78539816, 0.78539816), scale_ratio_range=(0.95, 1.05), shift_height=False):
        super().__init__(rot_range, scale_ratio_range, (0, 0, 0), shift_height)


@PIPELINES.register_module()
class PointsRangeFilter:
    """ref: uni3detr_sunrgbd.py:169 (mmdet3d PointsRangeFilter): survivors keep their order; every scene's segment keeps its offset,
    `count` says how many rows at its front are live."""

    def __init__(self, point_cloud_range):
        self.pcd_range = [float(v) for v in point_cloud_range]

    def __call__(self, batch):
        out, count = nv.points_range_filter(batch["points"], batch["scene_off"], self.pcd_range, out=batch["points"])
        batch["points"], batch["count"] = out, count
        return batch


@PIPELINES.register_module()
class PointSample:
    """ref: uni3detr_sunrgbd.py:171 (mmdet3d PointSample): every scene becomes exactly num_points rows."""

    def __init__(self, num_points, sample_range=None, replace=False):
        if sample_range is not None:
            raise NotImplementedError("sample_range is not used by any shipped Uni3DETR config")
        self.num_points = int(num_points)
        self._seed = None

    def __call__(self, batch):
        dev = batch["points"].device
        if self._seed is None or self._seed.device != dev:
            self._seed = torch.tensor([int(np.random.randint(0, 2 ** 62))], dtype=torch.int64, device=dev)
        else:
            self._seed += 0x9E3779B97F4A7C15 - (1 << 64)       # a new stream every call, device-side (capturable)
        B = batch["scene_off"].numel() - 1
        batch["points"] = nv.point_sample(batch["points"], batch["scene_off"], batch.get("count"), self.num_points, self._seed)
        batch["scene_off"] = torch.arange(0, (B + 1) * self.num_points, self.num_points, dtype=torch.int32, device=dev)
        batch.pop("count", None)
        return batch


@PIPELINES.register_module()
class ObjectRangeFilter:
    """ref: uni3detr_kitti_3classes.py / uni3detr_nuscenes.py train_pipeline (mmdet3d ObjectRangeFilter, recalled): ground-truth boxes
    whose BEV centre left (x0, y0, x1, y1) after flip / rotation / scale are dropped together with their labels, yaw is wrapped into
    [-pi, pi).  It runs AFTER the geometric augmentation, so with the augmentation on the device it has to be a device transform too:
    per scene, in place, order kept; `gt_count` says how many rows at the front of every scene's segment are live."""

    def __init__(self, point_cloud_range):
        r = [float(v) for v in point_cloud_range]
        self.bev_range = [r[0], r[1], r[3], r[4]]

    def __call__(self, batch):
        g = batch.get("gt_bboxes_3d")
        if g is None:
            return batch
        lab = batch.get("gt_labels_3d")
        if lab is not None and lab.dtype != torch.int32:
            lab = batch["gt_labels_3d"] = lab.to(torch.int32)
        if g.shape[0] == 0:
            # a batch without a single GT box (plausible for KITTI / nuScenes at 2-4 scenes per GPU): nothing to filter, and an empty
            # tensor has no device pointer to hand to the kernel
            batch["gt_count"] = torch.zeros(batch["gt_off"].numel() - 1, dtype=torch.int32, device=batch["gt_off"].device)
            return batch
        batch["gt_count"] = nv.boxes_range_filter(g, lab, batch["gt_off"], self.bev_range)
        return batch


def _replicate(x, off, views):
    """rows of every segment of x (segment i = rows off[i] .. off[i+1]), each repeated `views` times in a row: (rows, offsets) - one
    gather on the device, no host loop over the views.  Rows of x past off[-1] (spare capacity, as the sweep merge and ObjectSample
    leave it) are allowed: the output then has spare rows past the new off[-1] too (x's spare rows, then copies of its last row)."""
    dev = x.device
    n = int(x.shape[0])
    lens = (off[1:] - off[:-1]).long()
    lens_v = lens.repeat_interleave(views)
    off_v = torch.zeros(lens_v.numel() + 1, dtype=torch.long, device=dev)
    off_v[1:] = torch.cumsum(lens_v, 0)
    # one extra segment takes the n * views - off_v[-1] spare output rows (none for an exactly packed x), so that the repeat counts
    # always sum to output_size: repeat_interleave does not check that on the device
    counts = torch.cat([lens_v, (n * views - off_v[-1:]).clamp(min=0)])
    seg = torch.repeat_interleave(torch.arange(lens_v.numel() + 1, device=dev), counts, output_size=n * views)
    src = off.long()[seg // views] + torch.arange(n * views, device=dev) - off_v[seg]
    return x.index_select(0, src.clamp(max=max(n - 1, 0))), off_v.to(torch.int32)


@PIPELINES.register_module()
class MultiScaleFlipAug3D:
    """Test-time augmentation (mmdet3d MultiScaleFlipAug3D; the plugin's MultiRotScaleFlipAug3D, test_time_aug.py:10-125, adds
    `rotate_degree`, angles in radians).  A packed batch of B scenes becomes one packed batch of B*A scenes, scene-major, view-minor,
    the views enumerated in the reference's loop order (test_time_aug.py:84-107): rotation, scale, flip (`[True] if flip else [False]`),
    horizontal flip ([False, True] when enabled), vertical flip (likewise).  The scenes are replicated by one device gather; every
    view's draws are preset in the batch keys the inner transforms honour (pcd_horizontal_flip, pcd_vertical_flip, pcd_scale_factor,
    rot_degree -> GlobalRotScaleTrans's angle), and the inner transforms run once over the expanded batch.  batch["tta_views"] = A,
    batch["tta_params"] = f32 [B*A, 9] view table (flip_h, flip_v, sin, cos, angle, scale, 0, 0, 0): rotation and scale first, then the
    flips - the order of the inner pipelines (GlobalRotScaleTrans before RandomFlip3D); tta_forward_inputs() gives the reference's
    forward_test(points, img_metas) shape.  img_scale and flip_direction have no effect without images."""
    rotations = (0.0,)

    def __init__(self, transforms, img_scale=None, pts_scale_ratio=1, flip=False, flip_direction="horizontal", pcd_horizontal_flip=False,
                 pcd_vertical_flip=False, rotate_degree=None):
        self.pts_scale_ratio = [float(r) for r in pts_scale_ratio] if isinstance(pts_scale_ratio, (list, tuple)) else [float(pts_scale_ratio)]
        self.img_scale = img_scale if isinstance(img_scale, list) else [img_scale]
        self.rotate_degree = [float(r) for r in (rotate_degree if rotate_degree is not None else self.rotations)]
        self.flip, self.pcd_horizontal_flip, self.pcd_vertical_flip = bool(flip), bool(pcd_horizontal_flip), bool(pcd_vertical_flip)
        types = [t["type"] for t in transforms]
        flips = [i for i, t in enumerate(types) if t in ("RandomFlip3D", "UnifiedRandomFlip3D")]
        rots = [i for i, t in enumerate(types) if t in ("GlobalRotScaleTrans", "UnifiedRotScaleTrans")]
        if any(r != 0.0 for r in self.rotate_degree) and flips and (not rots or flips[0] < rots[0]):
            raise NotImplementedError("test-time rotations need GlobalRotScaleTrans before RandomFlip3D in the inner transforms")
        self.inner = DevicePipeline(transforms)

    def views(self):
        """[(rot, scale ratio, flip, horizontal, vertical)] in the reference's loop order (one entry per img_scale as well)."""
        fl = [True] if self.flip else [False]
        hf = [False, True] if self.flip and self.pcd_horizontal_flip else [False]
        vf = [False, True] if self.flip and self.pcd_vertical_flip else [False]
        return [(r, s, f, h, v) for r in self.rotate_degree for _ in self.img_scale for s in self.pts_scale_ratio for f in fl for h in hf
                for v in vf]

    def __call__(self, batch):
        views = self.views()
        A = len(views)
        B = batch["scene_off"].numel() - 1
        if views == [(0.0, 1.0, False, False, False)]:
            # the single identity view: the inner transforms run on the batch as they are (no replication, nothing preset)
            batch["tta_views"] = 1
            batch["tta_params"] = _params(dict(scene_off=batch["scene_off"], points=batch["points"]))
            return self.inner(batch)
        out = {k: v for k, v in batch.items() if k not in ("points", "scene_off", "count", "gt_bboxes_3d", "gt_off", "gt_labels_3d", "gt_count")}
        if "count" in batch:
            raise ValueError("MultiScaleFlipAug3D expects a packed batch (no `count`): it runs first in a test pipeline")
        out["points"], out["scene_off"] = _replicate(batch["points"], batch["scene_off"], A)
        if batch.get("gt_bboxes_3d") is not None:
            out["gt_bboxes_3d"], out["gt_off"] = _replicate(batch["gt_bboxes_3d"], batch["gt_off"], A)
            if batch.get("gt_labels_3d") is not None:
                out["gt_labels_3d"], _ = _replicate(batch["gt_labels_3d"], batch["gt_off"], A)
        rot = np.array([v[0] for v in views] * B, np.float32)
        sc = np.array([v[1] for v in views] * B, np.float32)
        out.update(rot_degree=rot, pcd_scale_factor=sc, flip=np.array([v[2] for v in views] * B, bool),
                   pcd_horizontal_flip=np.array([v[3] for v in views] * B, bool), pcd_vertical_flip=np.array([v[4] for v in views] * B, bool),
                   tta_views=A)
        out["tta_params"] = _params(dict(scene_off=out["scene_off"], points=out["points"], pcd_horizontal_flip=out["pcd_horizontal_flip"],
                                         pcd_vertical_flip=out["pcd_vertical_flip"], pcd_rotation_angle=rot, pcd_scale_factor=sc))
        return self.inner(out)


@PIPELINES.register_module()
class MultiRotScaleFlipAug3D(MultiScaleFlipAug3D):
    """ref: projects/mmdet3d_plugin/datasets/pipelines/test_time_aug.py:10-125 (rotate_degree: angles in radians)."""

    def __init__(self, transforms, img_scale=None, pts_scale_ratio=1, rotate_degree=(0.0,), flip=False, flip_direction="horizontal",
                 pcd_horizontal_flip=False, pcd_vertical_flip=False):
        super().__init__(transforms, img_scale, pts_scale_ratio, flip, flip_direction, pcd_horizontal_flip, pcd_vertical_flip,
                         rotate_degree=list(rotate_degree))


def tta_forward_inputs(batch):
    """an expanded batch (MultiScaleFlipAug3D) -> (points, img_metas) in the reference's forward_test shape: points[a][b] and
    img_metas[a][b] for view a of scene b, the metas holding pcd_scale_factor, pcd_horizontal_flip, pcd_vertical_flip, rot_degree and
    box_type_3d (views of the packed tensors: no copies)."""
    A = int(batch["tta_views"])
    pts = unpack_batch(batch)[0]
    B = len(pts) // A
    box_type = batch.get("box_type_3d", "Depth")
    points = [[pts[b * A + a] for b in range(B)] for a in range(A)]
    n = A * B
    sc = np.asarray(batch.get("pcd_scale_factor", np.ones(n)), np.float32)
    fh = np.asarray(batch.get("pcd_horizontal_flip", np.zeros(n, bool)), bool)
    fv = np.asarray(batch.get("pcd_vertical_flip", np.zeros(n, bool)), bool)
    rot = np.asarray(batch.get("rot_degree", np.zeros(n)), np.float32)
    metas = [[dict(pcd_scale_factor=float(sc[b * A + a]), pcd_horizontal_flip=bool(fh[b * A + a]), pcd_vertical_flip=bool(fv[b * A + a]),
                   rot_degree=float(rot[b * A + a]), box_type_3d=box_type) for b in range(B)] for a in range(A)]
    return points, metas


@OBJECT_AUG.register_module()
class ObjectSample:
    """ref: mmdet3d ObjectSample (recalled) with the plugin's UnifiedDataBaseSampler (projects/mmdet3d_plugin/datasets/pipelines/
    dbsampler.py: sample_all, sample_class_v2).  Per scene, in scene order, the host reads the scene's per-class GT count (one small
    device-to-host copy for the whole batch), computes sampled_num = round(rate * (max - count)) per class in sample_groups order and
    draws that many database rows from the class's BatchSampler; the draws go into batch["db_sampled"] (a list per scene of
    (rows, group index) arrays) and are replayed when already present.  The device then runs the collision test and sample_class_v2's
    greedy accept, removes the scene points inside an accepted box and pastes the accepted objects (points translated by their box,
    boxes and labels after the existing GT).  The sampled points go BEFORE the kept scene points (mmdet3d); UnifiedObjectSample puts
    them after (transform_3d.py:668).  The output is exactly packed: new scene_off / gt_off / gt_labels_3d, no count / gt_count (rows
    past scene_off[-1] / gt_off[-1] are spare capacity).  batch["db_accepted"]: int32 [K] device flags of the candidates."""
    sampled_first = True

    def __init__(self, db_sampler, sample_2d=False, gt_database=None, **kwargs):
        if sample_2d:
            raise NotImplementedError("ObjectSample: sample_2d (image pasting) is not supported on the device")
        if gt_database is None:
            raise ValueError("ObjectSample needs a GTDatabase (DevicePipeline(..., gt_database=...))")
        classes = db_sampler.get("classes")
        if classes is not None and list(classes) != list(gt_database.classes):
            raise ValueError(f"GTDatabase classes {gt_database.classes} differ from db_sampler.classes {list(classes)}")
        self.db = gt_database
        self.rate = float(db_sampler.get("rate", 1.0))
        self.groups = [(name, int(num)) for name, num in db_sampler["sample_groups"].items()]
        self.cat = {n: i for i, n in enumerate(gt_database.classes)}

    def draw(self, hist):
        """one scene's candidates: (database rows, group index) in sample_groups order (UnifiedDataBaseSampler.sample_all)."""
        rows, grp = [], []
        for gi, (name, mx) in enumerate(self.groups):
            n = int(np.round(self.rate * int(mx - int(hist[self.cat[name]]))).astype(np.int64))
            if n > 0 and len(self.db.rows.get(name, ())):
                r = self.db.sample(name, n)
                rows.append(r)
                grp.append(np.full(len(r), gi, np.int64))
        return (np.concatenate(rows) if rows else np.zeros(0, np.int64), np.concatenate(grp) if grp else np.zeros(0, np.int64))

    def __call__(self, batch):
        db, dev = self.db, batch["points"].device
        if batch.get("gt_labels_3d") is None:
            raise KeyError("ObjectSample needs gt_labels_3d in the batch")
        lab = batch["gt_labels_3d"] = batch["gt_labels_3d"].to(torch.int32).contiguous()
        gt, go, so = batch["gt_bboxes_3d"], batch["gt_off"], batch["scene_off"]
        if gt.shape[1] != db.box_dim or batch["points"].shape[1] != db.feat:
            raise ValueError(f"GTDatabase holds [{db.feat}]-feature points / [{db.box_dim}]-column boxes, the batch "
                             f"[{batch['points'].shape[1]}] / [{gt.shape[1]}]")
        B, C = so.numel() - 1, len(db.classes)
        stats = nv.objaug_stats(so, batch.get("count"), go, batch.get("gt_count"), lab, C)
        st = stats.cpu().numpy()                          # the one device-to-host copy
        n_live, g_live, hist = st[:B], st[B:2 * B], st[2 * B:].reshape(B, C)
        if "db_sampled" not in batch:
            batch["db_sampled"] = [self.draw(hist[b]) for b in range(B)]
        rows = [np.asarray(r, np.int64) for r, _ in batch["db_sampled"]]
        grps = [np.asarray(g, np.int64) for _, g in batch["db_sampled"]]
        ks = [len(r) for r in rows]
        if max(ks) > nv.OA_CAP:
            raise ValueError(f"ObjectSample: {max(ks)} candidates in one scene, at most {nv.OA_CAP}")
        ids_h = np.concatenate(rows).astype(np.int32)
        K = len(ids_h)
        sizes = db.obj_off_host[ids_h + 1] - db.obj_off_host[ids_h] if K else np.zeros(0, np.int64)
        stats_n, stats_g = stats[:B], stats[B:2 * B]
        if K:
            ids = torch.from_numpy(ids_h).to(dev)
            coff = torch.tensor(np.concatenate([[0], np.cumsum(ks)]).astype(np.int32), device=dev)
            cgrp = torch.from_numpy(np.concatenate(grps).astype(np.int32)).to(dev)
            acc = nv.objaug_accept(gt, go, stats_g, db.boxes, ids, coff, cgrp, max(ks))
        else:
            ids = coff = acc = torch.zeros((0,), dtype=torch.int32, device=dev)
        pts, so2, boxes, labels, go2 = nv.objaug_paste(
            batch["points"], so, stats_n, int(n_live.max(initial=0)), gt, lab, go, stats_g, nv._nz(db.points), db.obj_off, nv._nz(db.boxes),
            nv._nz(db.labels), ids, coff, acc, int(sizes.max(initial=0)), int(n_live.sum() + sizes.sum()), int(g_live.sum()) + K,
            self.sampled_first)
        batch.update(points=pts, scene_off=so2, gt_bboxes_3d=boxes, gt_off=go2, gt_labels_3d=labels, db_accepted=acc)
        batch.pop("count", None)
        batch.pop("gt_count", None)
        return batch


@OBJECT_AUG.register_module()
class UnifiedObjectSample(ObjectSample):
    """ref: transform_3d.py:591-786 - the sampled points go AFTER the kept scene points (:668)."""
    sampled_first = False

    def __init__(self, db_sampler, sample_2d=False, sample_method="depth", modify_points=False, gt_database=None, **kwargs):
        super().__init__(db_sampler, sample_2d, gt_database)


@OBJECT_AUG.register_module()
class ObjectNoise:
    """ref: mmdet3d ObjectNoise -> noise_per_object_v3_ (recalled) with global_rot_range = 0 (noise_per_box).  Per scene, in scene
    order, the host draws loc ~ N(0, translation_std) [G, num_try, 3], rot ~ U(rot_range) [G, num_try] and the (unused, zero-width)
    global rotation draw upstream makes as well, so the host RNG stream stays the reference's; the draws go into batch["object_noise"]
    (replayed when present).  The device takes, box by box, the lowest collision-free try, moves every point with the lowest-index
    original box holding it and adds loc / rot to the box; batch["object_noise_try"] = chosen try per box row (-1 = none)."""

    def __init__(self, translation_std=(0.25, 0.25, 0.25), global_rot_range=(0.0, 0.0), rot_range=(-0.15707963267, 0.15707963267),
                 num_try=100, **kwargs):
        if not isinstance(global_rot_range, (list, tuple, np.ndarray)):
            global_rot_range = [-global_rot_range, global_rot_range]
        if abs(global_rot_range[0] - global_rot_range[1]) >= 1e-3:
            raise NotImplementedError("ObjectNoise: global_rot_range != 0 (noise_per_box_v2_) is not supported on the device")
        if not isinstance(rot_range, (list, tuple, np.ndarray)):
            rot_range = [-rot_range, rot_range]
        if not isinstance(translation_std, (list, tuple, np.ndarray)):
            translation_std = [translation_std] * 3
        self.translation_std = np.asarray(translation_std, np.float32)
        self.rot_range, self.global_rot_range, self.num_try = list(rot_range), list(global_rot_range), int(num_try)

    def __call__(self, batch):
        g = batch.get("gt_bboxes_3d")
        if g is None:
            return batch
        so, go = batch["scene_off"], batch["gt_off"]
        B = so.numel() - 1
        go_h, so_h = go.cpu().numpy(), so.cpu().numpy()
        gc = batch["gt_count"].cpu().numpy() if "gt_count" in batch else np.diff(go_h)
        nc = batch["count"].cpu().numpy() if "count" in batch else np.diff(so_h)
        if "object_noise" not in batch:
            loc, rot = [], []
            for b in range(B):
                n = int(gc[b])
                loc.append(np.random.normal(scale=self.translation_std, size=[n, self.num_try, 3]).astype(np.float32))
                rot.append(np.random.uniform(self.rot_range[0], self.rot_range[1], size=[n, self.num_try]).astype(np.float32))
                np.random.uniform(self.global_rot_range[0], self.global_rot_range[1], size=[n, self.num_try])   # upstream's global draw
            batch["object_noise"] = dict(loc=loc, rot=rot)
        if int(gc.max(initial=0)) > nv.OA_CAP:
            raise ValueError(f"ObjectNoise: {int(gc.max())} boxes in one scene, at most {nv.OA_CAP}")
        G, T = g.shape[0], self.num_try
        if G == 0:
            batch["object_noise_try"] = torch.zeros((0,), dtype=torch.int32, device=g.device)
            return batch
        loc = np.zeros((G, T, 3), np.float32)
        rot = np.zeros((G, T), np.float32)
        for b in range(B):
            n = int(gc[b])
            loc[go_h[b]:go_h[b] + n] = batch["object_noise"]["loc"][b]
            rot[go_h[b]:go_h[b] + n] = batch["object_noise"]["rot"][b]
        dev = g.device
        g_live = torch.from_numpy(np.asarray(gc, np.int32)).to(dev)
        n_live = batch["count"] if "count" in batch else None
        batch["object_noise_try"] = nv.object_noise(batch["points"], so, n_live, int(nc.max(initial=0)), g, go, g_live,
                                                    torch.from_numpy(loc).to(dev), torch.from_numpy(rot).to(dev))
        return batch


@OBJECT_AUG.register_module()
class LoadPointsFromMultiSweeps:
    """ref: mmdet3d LoadPointsFromMultiSweeps (v1.0.0rc5, recalled), the second entry of the nuScenes train and test pipelines.  The host
    part is read_sweeps (the choice draw and the file reads, one record per scene) and pack_batch(..., sweeps=records) (one upload);
    this transform merges on the device (csrc/sweeps.hip): per scene the key frame with time 0, then the chosen sweeps in choice order
    (remove_close, rotation and translation into the key frame in float64, the time lag in column 4) or `sweeps_num` pad copies of the
    key frame, then the use_dim gather.  The output is exactly packed: new points / scene_off, rows past scene_off[-1] are spare
    capacity.  It runs on the packed key frames, before any other transform."""

    def __init__(self, sweeps_num=10, load_dim=5, use_dim=(0, 1, 2, 4), file_client_args=None, pad_empty_sweeps=False, remove_close=False,
                 test_mode=False):
        backend = (file_client_args or {}).get("backend", "disk")
        if backend != "disk" or any(k != "backend" for k in (file_client_args or {})):
            raise NotImplementedError(f"LoadPointsFromMultiSweeps: file_client_args {dict(file_client_args)} (only the disk backend)")
        if not isinstance(remove_close, bool) and float(remove_close) not in (0.0, 1.0):
            raise NotImplementedError(f"LoadPointsFromMultiSweeps: remove_close radius {remove_close} (upstream removes within 1.0)")
        self.sweeps_num, self.load_dim = int(sweeps_num), int(load_dim)
        self.use_dim = [int(d) for d in use_dim]
        if not 5 <= self.load_dim <= 8 or not 1 <= len(self.use_dim) <= 8 or not all(0 <= d < self.load_dim for d in self.use_dim):
            raise NotImplementedError(f"LoadPointsFromMultiSweeps: load_dim {load_dim} / use_dim {list(use_dim)} (5 <= load_dim <= 8, "
                                      "at most 8 columns)")
        self.pad_empty_sweeps, self.remove_close, self.test_mode = bool(pad_empty_sweeps), bool(remove_close), bool(test_mode)

    def choose(self, n_sweeps, rng=np.random):
        """upstream's choice rule: all sweeps when there are at most sweeps_num, the first sweeps_num in test mode, else a draw."""
        if n_sweeps <= self.sweeps_num:
            return np.arange(n_sweeps)
        if self.test_mode:
            return np.arange(self.sweeps_num)
        return rng.choice(n_sweeps, self.sweeps_num, replace=False)

    def __call__(self, batch):
        sw = batch["sweeps"]
        if "count" in batch:
            raise ValueError("LoadPointsFromMultiSweeps expects the packed key frames (no `count`): it runs first")
        pts = batch["points"]
        if sw["load_dim"] != self.load_dim or pts.shape[1] != self.load_dim or pts.shape[0] != sw["n_key"]:
            raise ValueError(f"LoadPointsFromMultiSweeps: the batch holds [{pts.shape[0]}, {pts.shape[1]}] key rows, the sweep record "
                             f"[{sw['n_key']}, {sw['load_dim']}], the entry load_dim {self.load_dim}")
        if any(r["sweeps_num"] != self.sweeps_num for r in sw["records"]):
            raise ValueError("LoadPointsFromMultiSweeps: the sweep records were read with another sweeps_num")
        batch["points"], batch["scene_off"] = nv.sweeps_merge(pts.contiguous(), sw["raw"], sw["seg_tab"], sw["seg_param"], sw["seg_chunk0"],
                                                              sw["scene_chunk0"], sw["n_chunks"], sw["out_rows"], self.use_dim,
                                                              self.remove_close)
        del batch["sweeps"]            # the raw rows and tables on the device are spent (stream-ordered free); sweep_choices stays
        return batch


def read_sweeps(info_like, entry_cfg, rng=np.random, choices=None):
    """The host part of LoadPointsFromMultiSweeps for one scene.  info_like: the dict NuScenesSweepDataset.get_data_info makes
    (`timestamp` in seconds, `sweeps`: dicts with data_path, timestamp in microseconds, sensor2lidar_rotation / _translation);
    entry_cfg: the pipeline entry.  Makes upstream's choice draw from `rng` (or reuses `choices`, e.g. a recorded
    batch["sweep_choices"][b]) and reads only the chosen files -> record dict(points=[float32 [n_j, load_dim]], rot f64 [S,3,3],
    trans f64 [S,3], dt f64 [S] (= timestamp - sweep timestamp / 1e6), choices int64 [S], pad, sweeps_num, load_dim)."""
    entry = LoadPointsFromMultiSweeps(**{k: v for k, v in entry_cfg.items() if k != "type"})
    sweeps, ts = info_like["sweeps"], info_like["timestamp"]
    pad = entry.pad_empty_sweeps and len(sweeps) == 0
    if pad:
        choices = np.zeros(0, np.int64)
    elif choices is None:
        choices = entry.choose(len(sweeps), rng)
    choices = np.asarray(choices, np.int64).reshape(-1)
    pts, rot, trans, dt = [], [], [], []
    for idx in choices:
        sweep = sweeps[int(idx)]
        pts.append(np.fromfile(sweep["data_path"], dtype=np.float32).reshape(-1, entry.load_dim))
        rot.append(np.asarray(sweep["sensor2lidar_rotation"], np.float64).reshape(3, 3))
        trans.append(np.asarray(sweep["sensor2lidar_translation"], np.float64).reshape(3))
        dt.append(ts - sweep["timestamp"] / 1e6)
    return dict(points=pts, rot=np.asarray(rot, np.float64).reshape(-1, 3, 3), trans=np.asarray(trans, np.float64).reshape(-1, 3),
                dt=np.asarray(dt, np.float64).reshape(-1), choices=choices, pad=bool(pad), sweeps_num=entry.sweeps_num,
                load_dim=entry.load_dim)


def _upload_sweeps(records, key_lens, feat, dev):
    """The segment tables of u3d_sweeps_merge and every raw sweep row, in one pinned buffer and one host-to-device copy."""
    if len(records) != len(key_lens):
        raise ValueError(f"{len(records)} sweep records for {len(key_lens)} scenes")
    ld = int(records[0]["load_dim"]) if records else feat
    if any(int(r["load_dim"]) != ld for r in records) or ld != feat:
        raise ValueError(f"sweep records of load_dim {[r['load_dim'] for r in records]} for key frames of {feat} columns")
    C = nv.SWEEPS_CHUNK
    seg, par, chunk0, scene_chunk0, raws = [], [], [0], [], []
    key_off = np.concatenate([[0], np.cumsum(key_lens)]).astype(np.int64)
    raw_rows = 0

    def add(kind, src, rows, p):
        seg.append((kind, src, rows))
        par.append(p)
        chunk0.append(chunk0[-1] + (rows + C - 1) // C)

    zero = np.zeros(nv.SWEEPS_NPARAM, np.float64)
    for b, r in enumerate(records):
        scene_chunk0.append(chunk0[-1])
        add(nv.SWEEP_SEG_KEY, int(key_off[b]), int(key_lens[b]), zero)
        if r["pad"]:
            for _ in range(int(r["sweeps_num"])):
                add(nv.SWEEP_SEG_PAD, int(key_off[b]), int(key_lens[b]), zero)
            continue
        for j, a in enumerate(r["points"]):
            a = np.asarray(a, np.float32).reshape(-1, ld)
            add(nv.SWEEP_SEG_SWEEP, raw_rows, a.shape[0], np.concatenate([r["rot"][j].reshape(9), r["trans"][j], [r["dt"][j]]]))
            raws.append(a)
            raw_rows += a.shape[0]
    scene_chunk0.append(chunk0[-1])
    out_rows = sum(e[2] for e in seg)
    if max(raw_rows, out_rows, int(key_off[-1]), chunk0[-1]) >= 2 ** 31:
        raise ValueError("sweep merge: 2^31 rows or more in the batch (the device offsets are int32)")
    S = len(seg)
    ints = np.concatenate([np.asarray(seg, np.int32).reshape(-1), np.asarray(chunk0, np.int32), np.asarray(scene_chunk0, np.int32)])
    nb_p, nb_i = S * nv.SWEEPS_NPARAM * 8, ints.size * 4
    nb_i_pad = (nb_i + 15) // 16 * 16
    buf = torch.empty((nb_p + nb_i_pad + raw_rows * ld * 4,), dtype=torch.uint8, pin_memory=True)
    host = buf.numpy()
    host[:nb_p].view(np.float64)[:] = np.asarray(par, np.float64).reshape(-1)
    host[nb_p:nb_p + nb_i].view(np.int32)[:] = ints
    if raw_rows:
        np.concatenate(raws, 0, out=host[nb_p + nb_i_pad:].view(np.float32).reshape(raw_rows, ld))
    d = buf.to(dev, non_blocking=True)                    # the one upload; the caching host allocator keeps buf until it is done
    di = d[nb_p:nb_p + nb_i].view(torch.int32)
    return dict(records=records, seg_param=d[:nb_p].view(torch.float64).reshape(S, nv.SWEEPS_NPARAM),
                seg_tab=di[:3 * S].reshape(S, 3), seg_chunk0=di[3 * S:4 * S + 1], scene_chunk0=di[4 * S + 1:],
                raw=d[nb_p + nb_i_pad:].view(torch.float32).reshape(raw_rows, ld), n_chunks=int(chunk0[-1]),
                out_rows=int(out_rows), n_key=int(key_off[-1]), load_dim=ld)


def _disk_backend_only(name, file_client_args):
    backend = (file_client_args or {}).get("backend", "disk")
    if backend != "disk" or any(k != "backend" for k in (file_client_args or {})):
        raise NotImplementedError(f"{name}: file_client_args {dict(file_client_args)} (only the disk backend)")


@OBJECT_AUG.register_module()
class LoadPointsFromFile:
    """ref: mmdet3d LoadPointsFromFile (v1.0.0rc5, RECALLED from its published behaviour - that version is not in the reference tree,
    parity is unpinned; the contract is INTEGRATION.md section P), the first entry of every shipped pipeline.  The host part is
    read_points (the file read, one record per scene) and pack_batch(None, ..., raw=records) (one upload); this transform runs on the
    device (csrc/points_load.hip): batch["raw_points"] [R, load_dim] -> batch["points"] [R, len(use_dim) + shift_height], the use_dim
    gather and, with shift_height, the column z - floor after the third selected one, floor = float32(np.percentile(z, 0.99)) per
    scene under the declared rule (linear interpolation in float64 between the exact order statistics of the float32 column).
    Publishes batch["floor_height"] (f32 [B], device) with shift_height and batch["color_dims"] (the last three columns) with
    use_color; drops raw_points and load_table.  It drops no row: scene_off stays as packed."""

    def __init__(self, coord_type, load_dim=6, use_dim=(0, 1, 2), shift_height=False, use_color=False, file_client_args=None):
        _disk_backend_only("LoadPointsFromFile", file_client_args)
        if str(coord_type).upper() not in ("CAMERA", "LIDAR", "DEPTH"):
            raise ValueError(f"LoadPointsFromFile: coord_type {coord_type!r}")
        self.coord_type, self.load_dim = str(coord_type).upper(), int(load_dim)
        self.use_dim = list(range(use_dim)) if isinstance(use_dim, int) else [int(d) for d in use_dim]
        self.shift_height, self.use_color = bool(shift_height), bool(use_color)
        feat = len(self.use_dim) + int(self.shift_height)
        if not 3 <= self.load_dim <= 8 or not 1 <= len(self.use_dim) or feat > 8:
            raise NotImplementedError(f"LoadPointsFromFile: load_dim {load_dim} / use_dim {use_dim} (3 <= load_dim <= 8, at most 8 output "
                                      "columns)")
        if max(self.use_dim) >= self.load_dim or min(self.use_dim) < 0:
            raise ValueError(f"LoadPointsFromFile: expect all used dimensions < {self.load_dim}, got {self.use_dim}")
        if self.shift_height and len(self.use_dim) < 3:
            raise ValueError("LoadPointsFromFile: shift_height needs x, y, z as the first three used dimensions")
        if self.use_color and len(self.use_dim) < 6:
            raise ValueError("LoadPointsFromFile: use_color needs at least six used dimensions (upstream asserts it)")
        self.feat = feat

    def __call__(self, batch):
        if "raw_points" not in batch:
            raise KeyError("LoadPointsFromFile needs batch['raw_points'] (pack_batch(None, ..., raw=records))")
        raw = batch["raw_points"]
        if raw.shape[1] != self.load_dim:
            raise ValueError(f"LoadPointsFromFile: the batch holds raw rows of {raw.shape[1]} columns, the entry load_dim {self.load_dim}")
        if raw.shape[0] >= 2 ** 31:
            raise NotImplementedError("LoadPointsFromFile: 2^31 rows or more in the batch")
        batch["points"], floor = nv.points_load(raw, batch["scene_off"], batch.get("load_table"), self.use_dim, self.shift_height)
        del batch["raw_points"]             # spent (stream-ordered free)
        batch.pop("load_table", None)
        if self.shift_height:
            batch["floor_height"], batch["height_dim"] = floor, 3
        if self.use_color:
            batch["color_dims"] = [self.feat - 3, self.feat - 2, self.feat - 1]
        return batch


@OBJECT_AUG.register_module()
class NormalizePointsColor:
    """ref: mmdet3d NormalizePointsColor (recalled): colour = (colour - color_mean) / 255.0 in float32, one launch in place over the
    three colour columns LoadPointsFromFile(use_color=True) published; color_mean None only divides."""

    def __init__(self, color_mean=None):
        if color_mean is not None and len(color_mean) != 3:
            raise ValueError(f"NormalizePointsColor: color_mean {color_mean!r} (three values)")
        self.color_mean = None if color_mean is None else [float(v) for v in color_mean]

    def __call__(self, batch):
        dims = batch["color_dims"]          # KeyError without it: upstream asserts the colour attribute
        if list(dims) != list(range(dims[0], dims[0] + 3)):
            raise NotImplementedError(f"NormalizePointsColor: colour columns {list(dims)} (three neighbouring columns)")
        nv.points_color_norm(batch["points"], dims[0], self.color_mean)
        return batch


# The LoadPointsFromFile entries of the shipped configs (configs/pipelines.py lists the loading entries by type only).
SHIPPED_LOAD_ENTRIES = {
    "sunrgbd": dict(type="LoadPointsFromFile", coord_type="DEPTH", shift_height=True, load_dim=6, use_dim=[0, 1, 2]),
    "scannet": dict(type="LoadPointsFromFile", coord_type="DEPTH", shift_height=False, load_dim=3, use_dim=[0, 1, 2]),
    "scannet_large": dict(type="LoadPointsFromFile", coord_type="DEPTH", shift_height=False, load_dim=3, use_dim=[0, 1, 2]),
    "kitti_3classes": dict(type="LoadPointsFromFile", coord_type="LIDAR", load_dim=4, use_dim=4),
    "kitti_car": dict(type="LoadPointsFromFile", coord_type="LIDAR", load_dim=4, use_dim=4),
    "nuscenes": dict(type="LoadPointsFromFile", coord_type="LIDAR", load_dim=5, use_dim=5),
}


def load_table(n_rows):
    """(i, g) per scene of NumPy's `linear` percentile at q = 0.99: pos = (n - 1) * (0.99 / 100), i = floor(pos), g = pos - i, in
    float64 -> f64 [B, 2] (an empty scene gets (0, 0); read_points refuses it when the height is asked for)."""
    n = np.asarray(n_rows, np.int64)
    pos = (np.maximum(n, 1) - 1).astype(np.float64) * np.true_divide(0.99, 100)
    i = np.floor(pos)
    return np.stack([i, pos - i], 1)


def read_points(path_or_info, entry_cfg):
    """The host part of LoadPointsFromFile for one scene: a path, or a dict with `pts_filename`; entry_cfg: the pipeline entry.
    Upstream's read (np.load for .npy, else np.fromfile(float32), then reshape(-1, load_dim)) and nothing else ->
    dict(raw=float32 [n, load_dim], load_dim=...)."""
    entry = LoadPointsFromFile(**{k: v for k, v in entry_cfg.items() if k != "type"})
    path = os.fspath(path_or_info["pts_filename"] if isinstance(path_or_info, dict) else path_or_info)
    a = np.load(path) if path.endswith(".npy") else np.fromfile(path, dtype=np.float32)
    a = np.ascontiguousarray(a, np.float32).reshape(-1, entry.load_dim)
    if entry.shift_height and a.shape[0] == 0:
        raise ValueError(f"LoadPointsFromFile: {path} holds no point, shift_height needs the percentile of its heights")
    return dict(raw=a, load_dim=entry.load_dim)


def _upload_raw(records, gt, labels, dev, pinned=None):
    """The raw file rows of every scene, the percentile table, scene_off and - where they come as NumPy arrays - the GT boxes and
    labels, in one pinned buffer and one host-to-device copy -> the batch entries.  pinned: a callable nbytes -> pinned uint8 tensor
    (a caller that owns its staging buffers, feeder.BatchFeeder); by default the caching host allocator keeps the buffer until the
    copy is done."""
    B = len(records)
    if B == 0:
        raise ValueError("pack_batch: no scene")
    ld = int(records[0]["load_dim"])
    if any(int(r["load_dim"]) != ld for r in records):
        raise ValueError(f"raw records of differing load_dim {[r['load_dim'] for r in records]}")
    lens = [int(r["raw"].shape[0]) for r in records]
    R = sum(lens)
    if R >= 2 ** 31:
        raise NotImplementedError("pack_batch: 2^31 raw rows or more in the batch (the device offsets are int32)")
    ints = [np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)]
    G, dim = 0, 7
    if gt is not None:
        if len(gt) != B:
            raise ValueError(f"{len(gt)} GT box arrays for {B} scenes")
        gl = [int(g.shape[0]) for g in gt]
        G, dim = sum(gl), int(gt[0].shape[1])
        ints.append(np.concatenate([[0], np.cumsum(gl)]).astype(np.int32))
        if labels is not None:
            ints.append(np.concatenate([np.asarray(l).reshape(-1) for l in labels]).astype(np.int32) if G else np.zeros(0, np.int32))
    ints = np.concatenate(ints)
    pad = lambda n: (n + 15) // 16 * 16            # noqa: E731
    nb_t, nb_i, nb_g = B * 16, pad(ints.size * 4), pad(G * dim * 4)
    total = nb_t + nb_i + nb_g + R * ld * 4
    buf = pinned(total) if pinned is not None else torch.empty((total,), dtype=torch.uint8, pin_memory=True)
    host = buf.numpy()
    host[:nb_t].view(np.float64)[:] = load_table(lens).reshape(-1)
    host[nb_t:nb_t + ints.size * 4].view(np.int32)[:] = ints
    if G:
        np.concatenate([np.asarray(g, np.float32) for g in gt], 0, out=host[nb_t + nb_i:nb_t + nb_i + G * dim * 4].view(np.float32).reshape(G, dim))
    if R:
        np.concatenate([r["raw"] for r in records], 0, out=host[nb_t + nb_i + nb_g:total].view(np.float32).reshape(R, ld))
    d = buf[:total].to(dev, non_blocking=True)            # the one upload
    di = d[nb_t:nb_t + ints.size * 4].view(torch.int32)
    out = dict(raw_points=d[nb_t + nb_i + nb_g:].view(torch.float32).reshape(R, ld), scene_off=di[:B + 1],
               load_table=d[:nb_t].view(torch.float64).reshape(B, 2))
    if gt is not None:
        out["gt_off"] = di[B + 1:2 * B + 2]
        out["gt_bboxes_3d"] = d[nb_t + nb_i:nb_t + nb_i + G * dim * 4].view(torch.float32).reshape(G, dim)
        if labels is not None:
            out["gt_labels_3d"] = di[2 * B + 2:2 * B + 2 + G]
    return out, lens


@OBJECT_AUG.register_module()
class PointShuffle:
    """ref: mmdet3d PointShuffle (recalled: BasePoints.shuffle, one torch.randperm per sample).  The torch stream cannot be replayed
    on the device, so the rule is PointSample's: the live rows of every scene (`count`, or the whole segment) go through a keyed
    pseudo-random permutation, out of place; the key comes from a device int64 seed that advances on every call (capturable).
    `count` and `scene_off` stay as they are."""

    def __init__(self):
        self._seed = None

    def __call__(self, batch):
        dev = batch["points"].device
        if self._seed is None or self._seed.device != dev:
            # one draw from the host stream, uploaded from pinned memory: no synchronising copy
            self._seed = torch.tensor([int(np.random.randint(0, 2 ** 62))], dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
        else:
            self._seed += 0x9E3779B97F4A7C15 - (1 << 64)
        batch["points"] = nv.point_shuffle(batch["points"], batch["scene_off"], batch.get("count"), self._seed)
        return batch


@OBJECT_AUG.register_module()
class ObjectNameFilter:
    """ref: mmdet3d ObjectNameFilter (recalled): the GT rows whose label is in range(len(classes)) are kept (LoadAnnotations3D labels
    names outside `classes` -1).  Per scene, in place, order kept, over the live prefix (`gt_count` after ObjectRangeFilter, or the
    whole segment); the survivors' count becomes `gt_count`.  7- and 9-column boxes."""

    def __init__(self, classes):
        self.classes = list(classes)
        self.labels = list(range(len(self.classes)))

    def __call__(self, batch):
        g = batch.get("gt_bboxes_3d")
        if g is None:
            return batch
        lab = batch["gt_labels_3d"]
        if lab.dtype != torch.int32 or not lab.is_contiguous():
            lab = batch["gt_labels_3d"] = lab.to(torch.int32).contiguous()
        if g.shape[0] == 0:
            batch["gt_count"] = torch.zeros(batch["gt_off"].numel() - 1, dtype=torch.int32, device=batch["gt_off"].device)
            return batch
        batch["gt_count"] = nv.boxes_label_filter(g, lab, batch["gt_off"], batch.get("gt_count"), len(self.classes))
        return batch


_PASSTHROUGH = {"LoadPointsFromFile", "LoadAnnotations3D", "DefaultFormatBundle3D", "Collect3D", "CollectUnified3D", "LoadPointsFromMultiSweeps",
                "ObjectNameFilter", "PointShuffle", "ObjectSample", "UnifiedObjectSample", "ObjectNoise", "NormalizePointsColor",
                "LoadImageFromFile", "LoadMultiViewImageFromFiles"}


class DevicePipeline:
    """The device-side part of a config's `train_pipeline` / `test_pipeline` list: loading / formatting entries (and the
    ground-truth database sampler, which needs the dataset's files) stay with the host loader and are skipped here unless the
    constructor opts them in."""

    def __init__(self, pipeline_cfg, gt_database=None, object_noise=False, sweeps=False, point_shuffle=False, name_filter=False, load=False,
                 normalize_color=False):
        """gt_database (uni3detr_amd.gtdb.GTDatabase): run ObjectSample / UnifiedObjectSample on the device; object_noise=True: run
        ObjectNoise on the device; sweeps=True: LoadPointsFromMultiSweeps (the batch then needs pack_batch(..., sweeps=...));
        point_shuffle=True: PointShuffle; name_filter=True: ObjectNameFilter; load=True: LoadPointsFromFile (the batch then comes from
        pack_batch(None, ..., raw=...)); normalize_color=True: NormalizePointsColor.  Without them these entries stay in `skipped`.
        load_cfg / sweeps_cfg: the opted-in loading entries as the config gives them (what read_points / read_sweeps take)."""
        self.transforms, self.skipped = [], []
        self.load_cfg = self.sweeps_cfg = None
        opt_in = {"ObjectNoise": object_noise, "LoadPointsFromMultiSweeps": sweeps, "PointShuffle": point_shuffle,
                  "ObjectNameFilter": name_filter, "LoadPointsFromFile": load, "NormalizePointsColor": normalize_color}
        for c in pipeline_cfg:
            if c["type"] == "LoadPointsFromFile" and load:
                self.load_cfg = dict(c)
            if c["type"] == "LoadPointsFromMultiSweeps" and sweeps:
                self.sweeps_cfg = dict(c)
            if c["type"] in ("ObjectSample", "UnifiedObjectSample") and gt_database is not None:
                if "db_sampler" not in c:
                    raise KeyError(f"pipeline entry {c['type']!r}: a device GT-paste needs the entry's db_sampler (sample_groups, rate)")
                self.transforms.append(OBJECT_AUG.build(c, gt_database=gt_database))
            elif opt_in.get(c["type"], False):
                self.transforms.append(OBJECT_AUG.build(c))
            elif c["type"] in PIPELINES:
                self.transforms.append(PIPELINES.build(c))
            elif c["type"] in _PASSTHROUGH:
                self.skipped.append(c["type"])
            else:
                raise KeyError(f"pipeline entry {c['type']!r}: neither a device transform nor a known host-side entry")

    def __call__(self, batch):
        for t in self.transforms:
            batch = t(batch)
        return batch


def pack_batch(points, gt_bboxes_3d=None, box_type_3d="Depth", height_dim=3, gt_labels_3d=None, *, sweeps=None, raw=None, device=None,
               pinned=None):
    """list of per-scene [n_i,F] tensors (+ list of [g_i,7|9] box tensors, + list of label tensors) on one device -> the batch dict
    the transforms take.  sweeps: one read_sweeps record per scene (the points are then the key frames): every raw sweep row goes up
    in one copy from pinned memory, batch["sweeps"] holds the records and the device tables until the merge drops them,
    batch["sweep_choices"] the choices.
    raw: one read_points record per scene, `points` must then be None (LoadPointsFromFile makes them on the device): all raw rows go
    up in one pinned buffer and one copy, batch["raw_points"] [R, load_dim], batch["scene_off"] from the row counts (the loader drops
    no row), batch["load_table"] f64 [B, 2] = (i, g) per scene (datapath.load_table).  The GT boxes / labels may then be NumPy arrays:
    they travel in the same copy.  device: where to (default: the GT tensors' device, else "cuda"); pinned: see _upload_raw.  With
    sweeps= as well the key frames are the loader's output, so the loader has to keep all load_dim columns of the sweep records."""
    if raw is not None:
        if points is not None:
            raise ValueError("pack_batch: raw= takes the place of points (pass points=None)")
        raw = list(raw)
        host_gt = gt_bboxes_3d is not None and all(isinstance(g, np.ndarray) for g in gt_bboxes_3d)
        if device is None:
            device = gt_bboxes_3d[0].device if gt_bboxes_3d is not None and len(gt_bboxes_3d) and not host_gt else "cuda"
        dev = torch.device(device)
        up, lens = _upload_raw(raw, gt_bboxes_3d if host_gt else None, gt_labels_3d if host_gt else None, dev, pinned)
        batch = dict(up, box_type_3d=box_type_3d, height_dim=height_dim)
        if host_gt:
            gt_bboxes_3d = None
        feat = int(raw[0]["load_dim"])
    else:
        dev = points[0].device
        lens = [int(p.shape[0]) for p in points]
        off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), device=dev)
        batch = dict(points=torch.cat([p.float() for p in points]).contiguous(), scene_off=off, box_type_3d=box_type_3d, height_dim=height_dim)
        feat = int(batch["points"].shape[1])
    if gt_bboxes_3d is not None:
        gl = [int(g.shape[0]) for g in gt_bboxes_3d]
        batch["gt_off"] = torch.tensor(np.concatenate([[0], np.cumsum(gl)]).astype(np.int32), device=dev)
        dim = gt_bboxes_3d[0].shape[1] if len(gt_bboxes_3d) else 7
        batch["gt_bboxes_3d"] = (torch.cat([g.float() for g in gt_bboxes_3d]).contiguous() if sum(gl)
                                 else torch.zeros((0, dim), dtype=torch.float32, device=dev))
        if gt_labels_3d is not None:
            batch["gt_labels_3d"] = (torch.cat([l.to(torch.int32) for l in gt_labels_3d]).contiguous() if sum(gl)
                                     else torch.zeros((0,), dtype=torch.int32, device=dev))
    if sweeps is not None:
        batch["sweeps"] = _upload_sweeps(list(sweeps), lens, feat, dev)
        batch["sweep_choices"] = [r["choices"] for r in sweeps]
    return batch


def unpack_batch(batch, labels=None):
    """batch dict -> (points list, Boxes3D list[, labels list]) as `Uni3DETR.forward_train` / `TrainStep.set_batch` take them
    (views of the packed tensors: no copies)."""
    from .plugin.structures import Boxes3D
    off = batch["scene_off"].tolist()
    pts = [batch["points"][off[b]:off[b + 1]] for b in range(len(off) - 1)]
    if "count" in batch:
        cnt = batch["count"].tolist()
        pts = [p[:c] for p, c in zip(pts, cnt)]
    out = [pts]
    if "gt_bboxes_3d" in batch:
        go = batch["gt_off"].tolist()
        gc = batch["gt_count"].tolist() if "gt_count" in batch else [go[b + 1] - go[b] for b in range(len(go) - 1)]     # ObjectRangeFilter survivors
        out.append([Boxes3D(batch["gt_bboxes_3d"][go[b]:go[b] + gc[b]]) for b in range(len(go) - 1)])
        if labels is None and "gt_labels_3d" in batch:
            labels = [batch["gt_labels_3d"][go[b]:go[b] + gc[b]].long() for b in range(len(go) - 1)]
    if labels is not None:
        out.append(labels)
    return tuple(out)
