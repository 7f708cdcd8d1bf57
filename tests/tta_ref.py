"""NumPy restatement of the test-time-augmentation merge (ref: projects/mmdet3d_plugin/core/merge_all_augs.py:9-98,
core/bbox/util.py:82-102) and of the upstream pieces it calls, recalled - parity unpinned where it rests on recall:

  * mmdet3d box `flip` / `scale` / `rotate` (Depth and LiDAR, with velocities) in the project's convention, the one
    oracle/datapath.py::augment_boxes restates (flip axes of mmdet3d v1.0, rotation x' = x cos - y sin, yaw + angle, velocities flip,
    rotate and scale with the frame);
  * `xywhr2xyxyr`, mmcv `nms_bev` (score sort, the xyxyr -> xywhr way back, greedy rotated NMS suppressing at IoU > thr) and
    `bbox3d2result`;
  * the merge rules the product declares on top of the reference: candidates in view order, non-finite scores dropped, stable sorts
    (equal scores go to the lower concatenated index), classes ascending, empty classes skipped, the first min(max_num, kept).

`Boxes` is also the stand-in box class under which the reference's own merge_all_aug_bboxes_3d / bbox3d_mapping_back run in
tests/test_tta_cpu.py.
"""
import math

import numpy as np
import torch

from oracle.boxes import rotated_intersection_area

DEPTH, LIDAR = 0, 1
F32 = np.float32


def flip_boxes(b, direction, coord):
    """mmdet3d `flip(bev_direction)` in f32: Depth horizontal x -> -x, yaw -> pi - yaw, vertical y -> -y, yaw -> -yaw; LiDAR horizontal
    y -> -y, yaw -> -yaw, vertical x -> -x, yaw -> pi - yaw; velocities mirror with the frame."""
    b = np.array(b, F32, copy=True)
    pi = F32(np.pi)
    ax = 0 if (coord == DEPTH) == (direction == "horizontal") else 1
    b[:, ax] = -b[:, ax]
    if b.shape[1] >= 9:
        b[:, 7 + ax] = -b[:, 7 + ax]
    b[:, 6] = (-b[:, 6] + pi) if ax == 0 else -b[:, 6]
    return b


def scale_boxes(b, s):
    """mmdet3d `scale`: centres, sizes and velocities times s."""
    b = np.array(b, F32, copy=True)
    s = F32(s)
    b[:, :6] *= s
    if b.shape[1] >= 9:
        b[:, 7:9] *= s
    return b


def rotate_boxes(b, angle):
    """rotation by angle about z: (x, y) -> (x cos - y sin, x sin + y cos), yaw + angle, velocities rotate too."""
    b = np.array(b, F32, copy=True)
    a = F32(angle)
    s, c = F32(np.sin(a)), F32(np.cos(a))
    x, y = b[:, 0].copy(), b[:, 1].copy()
    b[:, 0], b[:, 1] = x * c - y * s, x * s + y * c
    b[:, 6] = b[:, 6] + a
    if b.shape[1] >= 9:
        vx, vy = b[:, 7].copy(), b[:, 8].copy()
        b[:, 7], b[:, 8] = vx * c - vy * s, vx * s + vy * c
    return b


def mapping_back(b, rot, scale, fh, fv, coord):
    """bbox3d_mapping_back (util.py:82-102): flip horizontal, flip vertical, scale 1/s, rotate -rot."""
    if fh:
        b = flip_boxes(b, "horizontal", coord)
    if fv:
        b = flip_boxes(b, "vertical", coord)
    b = scale_boxes(b, 1.0 / float(scale))
    return rotate_boxes(b, -float(rot))


def xywhr2xyxyr(bev):
    """f32 [n, 5] (x, y, w, h, r) -> (x1, y1, x2, y2, r)"""
    bev = np.asarray(bev, F32)
    hw, hh = bev[:, 2] / F32(2), bev[:, 3] / F32(2)
    return np.stack([bev[:, 0] - hw, bev[:, 1] - hh, bev[:, 0] + hw, bev[:, 1] + hh, bev[:, 4]], 1).astype(F32)


def xyxyr_back(b):
    """nms_bev's way back to (cx, cy, w, h, r), f32"""
    b = np.asarray(b, F32)
    return np.stack([(b[:, 0] + b[:, 2]) / F32(2), (b[:, 1] + b[:, 3]) / F32(2), b[:, 2] - b[:, 0], b[:, 3] - b[:, 1], b[:, 4]], 1).astype(F32)


def iou_bev(p, q):
    """rotated BEV IoU of two (cx, cy, w, h, r) rows, float64"""
    p, q = [float(v) for v in p], [float(v) for v in q]
    a1, a2 = p[2] * p[3], q[2] * q[3]
    if a1 <= 0 or a2 <= 0:
        return 0.0
    inter = rotated_intersection_area((0.0, 0.0, p[2], p[3], p[4]), (q[0] - p[0], q[1] - p[1], q[2], q[3], q[4]))
    return inter / max(a1 + a2 - inter, 1e-8)


def nms_bev(xyxyr, scores, thr):
    """mmcv nms_bev (recalled): kept indices in selection order; the sort is stable here (declared tie rule)."""
    scores = np.asarray(scores)
    order = np.argsort(-scores.astype(np.float64), kind="stable")
    rows = xyxyr_back(np.asarray(xyxyr, F32)[order])
    removed = np.zeros(len(order), bool)
    rad = 0.5 * np.hypot(rows[:, 2].astype(np.float64), rows[:, 3].astype(np.float64))
    keep = []
    for i in range(len(order)):
        if removed[i]:
            continue
        keep.append(order[i])
        d = np.hypot(rows[i + 1:, 0].astype(np.float64) - rows[i, 0], rows[i + 1:, 1].astype(np.float64) - rows[i, 1])
        for j in (i + 1 + np.nonzero(d < rad[i] + rad[i + 1:] + 1e-6)[0]):       # circumcircles apart: no intersection
            if not removed[j] and iou_bev(rows[i], rows[j]) > thr:
                removed[j] = True
    return np.asarray(keep, np.int64)


def bbox3d2result(bboxes, scores, labels):
    return dict(boxes_3d=bboxes, scores_3d=scores, labels_3d=labels)


def merge(views, params, coord, nms_thr=0.1, max_num=500):
    """One sample.  views: per view (boxes [n, 7|9], scores [n], labels [n]); params: per view (rot, scale, fh, fv)
    -> (boxes, scores, labels) numpy, the merged result."""
    dim = next((np.asarray(v[0]).shape[1] for v in views if np.asarray(v[0]).ndim == 2), 7)
    rb, rs, rl = [], [], []
    for (b, s, l), (rot, sc, fh, fv) in zip(views, params):
        b = np.asarray(b, F32).reshape(-1, dim)
        rb.append(mapping_back(b, rot, sc, fh, fv, coord))
        rs.append(np.asarray(s, F32).reshape(-1))
        rl.append(np.asarray(l, np.int64).reshape(-1))
    boxes, scores, labels = np.concatenate(rb), np.concatenate(rs), np.concatenate(rl)
    ok = np.isfinite(scores)
    boxes, scores, labels = boxes[ok], scores[ok], labels[ok]
    if len(labels) == 0:
        return np.zeros((0, dim), F32), np.zeros(0, F32), np.zeros(0, np.int64)
    xyxyr = xywhr2xyxyr(boxes[:, [0, 1, 3, 4, 6]])
    mb, ms, ml = [], [], []
    for c in range(int(labels.max()) + 1):
        idx = np.nonzero(labels == c)[0]
        if len(idx) == 0:
            continue
        sel = idx[nms_bev(xyxyr[idx], scores[idx], nms_thr)]
        mb.append(boxes[sel])
        ms.append(scores[sel])
        ml.append(labels[sel])
    mb, ms, ml = np.concatenate(mb), np.concatenate(ms), np.concatenate(ml)
    order = np.argsort(-ms.astype(np.float64), kind="stable")[:min(max_num, len(ms))]
    return mb[order], ms[order], ml[order]


def same_class_ious(views, params, coord):
    """every same-class BEV IoU among a sample's mapped-back candidates (to keep random tests away from the threshold)"""
    dim = np.asarray(views[0][0]).shape[1]
    b = np.concatenate([mapping_back(np.asarray(v[0], F32).reshape(-1, dim), *p, coord) for v, p in zip(views, params)])
    l = np.concatenate([np.asarray(v[2]).reshape(-1) for v in views])
    rows = xyxyr_back(xywhr2xyxyr(b[:, [0, 1, 3, 4, 6]])).astype(np.float64)
    rad = 0.5 * np.hypot(rows[:, 2], rows[:, 3])
    out = []
    for i in range(len(l)):
        d = np.hypot(rows[i + 1:, 0] - rows[i, 0], rows[i + 1:, 1] - rows[i, 1])
        for j in (i + 1 + np.nonzero((d < rad[i] + rad[i + 1:] + 1e-6) & (l[i + 1:] == l[i]))[0]):
            out.append(iou_bev(rows[i], rows[j]))
    return np.asarray(out)


class Boxes:
    """Stand-in for mmdet3d's Depth / LiDAR box classes, enough for the reference's merge: clone, flip, scale, rotate, cat, bev,
    indexing, len, to."""
    coord = DEPTH

    def __init__(self, tensor, box_dim=None):
        self.tensor = torch.as_tensor(tensor, dtype=torch.float32).clone()
        if self.tensor.numel() == 0:
            self.tensor = self.tensor.reshape(0, box_dim or 7)

    def _set(self, a):
        self.tensor = torch.from_numpy(np.ascontiguousarray(a, F32))

    def clone(self):
        return type(self)(self.tensor)

    def flip(self, bev_direction="horizontal", points=None):
        self._set(flip_boxes(self.tensor.numpy(), bev_direction, self.coord))

    def scale(self, s):
        self._set(scale_boxes(self.tensor.numpy(), float(s)))

    def rotate(self, angle, points=None):
        self._set(rotate_boxes(self.tensor.numpy(), float(angle)))

    @classmethod
    def cat(cls, boxes_list):
        return cls(torch.cat([b.tensor for b in boxes_list]))

    @property
    def bev(self):
        return self.tensor[:, [0, 1, 3, 4, 6]]

    def __getitem__(self, item):
        t = self.tensor[item]
        return type(self)(t.reshape(1, -1) if t.dim() == 1 else t)

    def __len__(self):
        return self.tensor.shape[0]

    def to(self, *a, **k):
        return type(self)(self.tensor.to(*a, **k))


class DepthBoxes(Boxes):
    coord = DEPTH


class LiDARBoxes(Boxes):
    coord = LIDAR


def torch_xywhr2xyxyr(bev):
    return torch.from_numpy(xywhr2xyxyr(bev.numpy()))


def torch_nms_bev(boxes, scores, thresh, pre_max_size=None, post_max_size=None):
    return torch.from_numpy(nms_bev(boxes.numpy(), scores.numpy(), thresh))


def torch_bbox3d2result(bboxes, scores, labels, attrs=None):
    return bbox3d2result(bboxes.to("cpu"), scores.cpu(), labels.cpu())


def yaw_close(a, b, tol):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    d = (d + math.pi) % (2 * math.pi) - math.pi
    return np.abs(d) <= tol
