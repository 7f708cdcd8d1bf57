"""Indoor 3-D detection evaluation: per-class AP and recall at 3-D IoU thresholds (SUN RGB-D / ScanNet `evaluation` of the shipped
indoor configs).

Semantics are those of the reference's `indoor_eval_ov` with every class seen, i.e. mmdet3d's `indoor_eval`
(ref: projects/mmdet3d_plugin/core/indoor_eval.py):
  * predictions are bottom-centre (x, y, z, dx, dy, dz, yaw) boxes (the first 7 columns of `Uni3DETRHead.get_bboxes`); GT are
    `gt_boxes_upright_depth`, gravity-centre, moved to bottom-centre; a 6-column GT box has yaw 0.  `axis_aligned_lw=True` replaces the
    GT dims by the axis-aligned extent of the box corners and keeps the yaw column, as the reference does;
  * IoU is the rotated 3-D IoU of `DepthInstance3DBoxes.overlaps` (the arithmetic of `pp_iou3d` in csrc/box_iou.h);
  * a detection is compared with the GT of its class in its scene only; its best GT is the FIRST maximal IoU (strict '>' from -inf,
    a NaN never wins); at threshold t it is a TP iff iou_max > t and that GT was not taken by an earlier-ranked detection;
  * detections are ranked per class by descending score across all scenes.  The reference's `np.argsort(-confidence)` is not stable, so
    its order among equal scores depends on the platform; here ties are STABLE: by (scene index, position in the scene's list);
  * AP is the 'area' mode of `average_precision` in float64, stored as float32; a class with GT but no predictions gets AP 0 and recall
    0, a predicted class without GT anywhere gets NaN for both; NaNs are left out of mAP / mAR; non-finite scores raise ValueError.

Two implementations of the same result: the device path (csrc/eval.hip, through `native.eval_indoor`; the one ATen op of substance is
the stable sort of the 64-bit (class, score) keys) and a float64 NumPy restatement for `device="cpu"` (saved results on a machine
without a GPU).
"""
import numpy as np
import torch

from .eval_common import DetBuffer, as_tensor, default_device, fit_columns, invalid_device, invalid_host, offsets, print_log, to_numpy

_EPS = np.finfo(np.float64).eps
# the messages of the input checks: a non-finite score, a negative label, a label that num_classes does not cover
ERRORS = ("indoor evaluation: detection scores must be finite", "indoor evaluation: labels must be non-negative",
          "indoor evaluation: labels must be below num_classes = {}")


# --------------------------------------------------------------------------------------------------
# input preparation
# --------------------------------------------------------------------------------------------------
def _gt_bottom_boxes(gt_boxes_upright_depth, axis_aligned_lw=False):
    """gravity-centre GT [n,6|7] -> float32 [n,7] bottom-centre (DepthInstance3DBoxes(..., origin=(0.5, 0.5, 0.5)).tensor)."""
    g = np.asarray(gt_boxes_upright_depth)
    if g.size == 0:
        return np.zeros((0, 7), np.float32)
    g = g.reshape(g.shape[0], -1)
    if axis_aligned_lw and g.shape[1] >= 7:
        # the extent of the 8 corners of the (float32) box: |dx cos| + |dy sin|, |dx sin| + |dy cos|, dz; the yaw column stays
        b = g[:, :7].astype(np.float32).astype(np.float64)
        c, s = np.abs(np.cos(b[:, 6])), np.abs(np.sin(b[:, 6]))
        g = g.copy()
        g[:, 3] = b[:, 3] * c + b[:, 4] * s
        g[:, 4] = b[:, 3] * s + b[:, 4] * c
    t = np.zeros((g.shape[0], 7), np.float32)
    t[:, : min(7, g.shape[1])] = g[:, :7].astype(np.float32)
    t[:, 2] = t[:, 2] + t[:, 5] * np.float32(-0.5)
    return t


def _flatten_dt(dt_annos):
    buf = DetBuffer(7, torch.float32, "cpu")
    for d in dt_annos:
        buf.add(d)
    boxes, scores, labels, _ = buf.cat()
    return boxes.numpy(), scores.numpy(), labels.numpy(), np.asarray(buf.counts, np.int64)


def _flatten_gt(gt_annos, axis_aligned_lw):
    boxes, labels, counts = [], [], []
    for g in gt_annos:
        if g["gt_num"] != 0:
            b = _gt_bottom_boxes(g["gt_boxes_upright_depth"], axis_aligned_lw)
            lab = np.asarray(g["class"]).astype(np.int64).reshape(-1)
        else:
            b, lab = np.zeros((0, 7), np.float32), np.zeros(0, np.int64)
        boxes.append(b)
        labels.append(lab)
        counts.append(b.shape[0])
    return (np.concatenate(boxes) if boxes else np.zeros((0, 7), np.float32), np.concatenate(labels) if labels else np.zeros(0, np.int64),
            np.asarray(counts, np.int64))


def _raise_invalid(flags, num_classes):
    """flags: eval_common.invalid_host / invalid_device over the detection and GT labels"""
    for bad, msg in zip(flags, ERRORS):
        if bad:
            raise ValueError(msg.format(num_classes))


# --------------------------------------------------------------------------------------------------
# host path (float64 NumPy)
# --------------------------------------------------------------------------------------------------
def rect_corners(cx, cy, w, h, a):
    """[P,4,2] counter-clockwise corners (pp_rect)."""
    c, s = np.cos(a), np.sin(a)
    sx = np.array([-0.5, 0.5, 0.5, -0.5])
    sy = np.array([-0.5, -0.5, 0.5, 0.5])
    x, y = sx[None, :] * w[:, None], sy[None, :] * h[:, None]
    return np.stack([cx[:, None] + x * c[:, None] - y * s[:, None], cy[:, None] + x * s[:, None] + y * c[:, None]], -1)


def rect_inter_area(a, b):
    """Area of rectangle a clipped by rectangle b (Sutherland-Hodgman over b's 4 edges, the clip order of pp_inter_area), [P]."""
    P = a.shape[0]
    poly = np.zeros((P, 8, 2))
    poly[:, :4] = a
    n = np.full(P, 4)
    slots = np.arange(8)
    for e in range(4):
        A, B = b[:, e], b[:, (e + 1) % 4]
        nxt = (slots[None, :] + 1) % np.maximum(n, 1)[:, None]
        q = np.take_along_axis(poly, nxt[..., None].repeat(2, -1), 1)
        valid = slots[None, :] < n[:, None]
        ex, ey = (B[:, 0] - A[:, 0])[:, None], (B[:, 1] - A[:, 1])[:, None]
        sp = ex * (poly[..., 1] - A[:, 1:2]) - ey * (poly[..., 0] - A[:, 0:1])
        sq = ex * (q[..., 1] - A[:, 1:2]) - ey * (q[..., 0] - A[:, 0:1])
        keep = valid & (sp >= 0)
        cross = valid & ((sp >= 0) != (sq >= 0))
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(cross, sp / np.where(cross, sp - sq, 1.0), 0.0)
        inter = poly + t[..., None] * (q - poly)
        cand = np.stack([poly, inter], 2).reshape(P, 16, 2)
        m = np.stack([keep, cross], 2).reshape(P, 16)
        order = np.argsort(~m, axis=1, kind="stable")[:, :8]          # a convex quad clipped 4 times keeps <= 8 vertices
        poly = np.take_along_axis(cand, order[..., None].repeat(2, -1), 1)
        n = m.sum(1)
    nxt = (slots[None, :] + 1) % np.maximum(n, 1)[:, None]
    q = np.take_along_axis(poly, nxt[..., None].repeat(2, -1), 1)
    cr = np.where(slots[None, :] < n[:, None], poly[..., 0] * q[..., 1] - q[..., 0] * poly[..., 1], 0.0)
    return np.where(n >= 3, np.abs(cr.sum(1)) * 0.5, 0.0)


def box_iou3d_pairs(p, q, chunk=1 << 16):
    """Rotated 3-D IoU of box pairs (p[i], q[i]), float64 [P]: the arithmetic of DepthInstance3DBoxes.overlaps (BEV widths clamped to
    1e-4, ov_bev = iou2d (a1 + a2) / (1 + iou2d), height overlap from the bottom z, ov / max(v1 + v2 - ov, 1e-8))."""
    p = np.asarray(p, np.float64).reshape(-1, 7)
    q = np.asarray(q, np.float64).reshape(-1, 7)
    out = np.empty(p.shape[0], np.float64)
    for s in range(0, p.shape[0], chunk):
        a, b = p[s:s + chunk], q[s:s + chunk]
        w1, h1 = np.maximum(a[:, 3], 1e-4), np.maximum(a[:, 4], 1e-4)
        w2, h2 = np.maximum(b[:, 3], 1e-4), np.maximum(b[:, 4], 1e-4)
        a1, a2 = w1 * h1, w2 * h2
        z = np.zeros(a.shape[0])
        ra = rect_corners(z, z, w1, h1, a[:, 6])
        rb = rect_corners(b[:, 0] - a[:, 0], b[:, 1] - a[:, 1], w2, h2, b[:, 6])
        inter = rect_inter_area(ra, rb)
        with np.errstate(divide="ignore", invalid="ignore"):
            iou2d = np.where((a1 >= 1e-14) & (a2 >= 1e-14), inter / (a1 + a2 - inter), 0.0)
            ov_bev = iou2d * (a1 + a2) / (1.0 + iou2d)
            top = np.minimum(a[:, 2] + a[:, 5], b[:, 2] + b[:, 5])
            bot = np.maximum(a[:, 2], b[:, 2])
            ov = ov_bev * np.maximum(top - bot, 0.0)
            v1, v2 = a[:, 3] * a[:, 4] * a[:, 5], b[:, 3] * b[:, 4] * b[:, 5]
            out[s:s + chunk] = ov / np.maximum(v1 + v2 - ov, 1e-8)
    return out


def bbox_overlaps_3d(b1, b2):
    """[N,M] rotated 3-D IoU matrix (float64) of bottom-centre boxes."""
    b1, b2 = np.asarray(b1, np.float64).reshape(-1, 7), np.asarray(b2, np.float64).reshape(-1, 7)
    n, m = b1.shape[0], b2.shape[0]
    return box_iou3d_pairs(np.repeat(b1, m, 0), np.tile(b2, (n, 1))).reshape(n, m)


def host_iou_argmax(det_boxes, det_labels, det_off, gt_boxes, gt_labels, gt_off):
    """Per detection: (iou_max float64 (-inf without same-class GT in its scene), jmax int64 (global GT index of the first maximum, -1))."""
    nd, ns = det_boxes.shape[0], len(det_off) - 1
    C = int(max(det_labels.max(initial=-1), gt_labels.max(initial=-1))) + 1
    det_scene = np.repeat(np.arange(ns), np.diff(det_off))
    gt_scene = np.repeat(np.arange(ns), np.diff(gt_off))
    gkey = gt_scene * C + gt_labels
    gorder = np.argsort(gkey, kind="stable")                     # within a key: ascending GT index (the reference's j order)
    gks = gkey[gorder]
    dkey = det_scene * C + det_labels
    lo, hi = np.searchsorted(gks, dkey, "left"), np.searchsorted(gks, dkey, "right")
    cnt = hi - lo
    start = np.zeros(nd, np.int64)
    start[1:] = np.cumsum(cnt)[:-1]
    P = int(cnt.sum())
    pair_det = np.repeat(np.arange(nd), cnt)
    pair_gt = gorder[np.arange(P) - np.repeat(start, cnt) + np.repeat(lo, cnt)]
    iou_max = np.full(nd, -np.inf)
    jmax = np.full(nd, -1, np.int64)
    if P == 0:
        return iou_max, jmax
    v = box_iou3d_pairs(det_boxes[pair_det], gt_boxes[pair_gt])
    v = np.where(np.isnan(v), -np.inf, v)
    has = cnt > 0
    seg_max = np.maximum.reduceat(v, start[has])
    iou_max[has] = seg_max
    pos = np.where((v == iou_max[pair_det]) & (v > -np.inf), np.arange(P), P)
    first = np.minimum.reduceat(pos, start[has])
    jm = np.full(first.shape, -1, np.int64)
    ok = first < P
    jm[ok] = pair_gt[first[ok]]
    jmax[has] = jm
    return iou_max, jmax


def host_rank(scores, labels):
    """Rank order: class ascending, score descending, ties by input (= scene, position) order."""
    s = np.asarray(scores, np.float32).astype(np.float64)
    return np.lexsort((np.arange(s.shape[0]), -s, np.asarray(labels)))


def host_tp(order, iou_max, jmax, iou_thrs):
    """TP flags [T, N] in rank order: iou_max > t and the earliest-ranked such detection with its jmax (the reference's greedy loop)."""
    iou_r, j_r = np.asarray(iou_max, np.float64)[order], np.asarray(jmax)[order]
    tp = np.zeros((len(iou_thrs), order.shape[0]), np.uint8)
    for t, thr in enumerate(iou_thrs):
        elig = np.nonzero((iou_r > float(np.float32(thr))) & (j_r >= 0))[0]
        _, first = np.unique(j_r[elig], return_index=True)
        tp[t, elig[first]] = 1
    return tp


def _average_precision(recall, precision):
    """'area' mode of the reference's average_precision for one curve -> float32."""
    mrec = np.concatenate([[0.0], recall, [1.0]])
    mpre = np.concatenate([[0.0], precision, [0.0]])
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    ind = np.where(mrec[1:] != mrec[:-1])[0]
    return np.float32(np.sum((mrec[ind + 1] - mrec[ind]) * mpre[ind + 1]))


def host_ap(tp, labels_ranked, npos, num_classes):
    """-> ap float32 [T, C], final recall float64 [T, C] (curves in float64 as the reference's eval_det_cls)."""
    T = tp.shape[0]
    ap = np.zeros((T, num_classes), np.float32)
    rec = np.zeros((T, num_classes), np.float64)
    lo = np.searchsorted(labels_ranked, np.arange(num_classes), "left")
    hi = np.searchsorted(labels_ranked, np.arange(num_classes), "right")
    with np.errstate(divide="ignore", invalid="ignore"):
        for c in range(num_classes):
            if hi[c] == lo[c]:
                continue
            for t in range(T):
                f = tp[t, lo[c]:hi[c]].astype(np.float64)
                tpc, fpc = np.cumsum(f), np.cumsum(1.0 - f)
                recall = tpc / float(npos[c])
                precision = tpc / np.maximum(tpc + fpc, _EPS)
                ap[t, c] = _average_precision(recall, precision)
                rec[t, c] = recall[-1]
    return ap, rec


def _host_eval(det_boxes, det_scores, det_labels, det_off, gt_boxes, gt_labels, gt_off, num_classes, iou_thrs):
    iou_max, jmax = host_iou_argmax(det_boxes, det_labels, det_off, gt_boxes, gt_labels, gt_off)
    order = host_rank(det_scores, det_labels)
    tp = host_tp(order, iou_max, jmax, iou_thrs)
    npos = np.bincount(gt_labels, minlength=num_classes)[:num_classes]
    ndet = np.bincount(det_labels, minlength=num_classes)[:num_classes]
    ap, rec = host_ap(tp, det_labels[order], npos, num_classes)
    return dict(iou_max=iou_max, jmax=jmax, order=order, tp=tp, npos=npos, ndet=ndet, ap=ap, rec=rec)


# --------------------------------------------------------------------------------------------------
# device path
# --------------------------------------------------------------------------------------------------
def _device_eval(det_boxes, det_scores, det_labels, det_off, gt_boxes, gt_labels, gt_off, num_classes, iou_thrs, device):
    """All inputs are torch tensors on `device` (boxes f32 [.,7], scores f32, labels int32, offsets int32)."""
    from . import native as nv
    _raise_invalid(invalid_device(det_scores, (det_labels, gt_labels), num_classes), num_classes)
    thr = torch.tensor([float(t) for t in iou_thrs], dtype=torch.float32, device=device)
    r = nv.eval_indoor(det_boxes, det_scores, det_labels, det_off, gt_boxes, gt_labels, gt_off, num_classes, thr)
    seg = r["seg"].cpu().numpy()
    r["npos"], r["ndet"] = r["npos"].cpu().numpy().astype(np.int64), (seg[:, 1] - seg[:, 0]).astype(np.int64)
    r["ap"], r["rec"] = r["ap"].cpu().numpy(), r["rec"].cpu().numpy()
    return r


def evaluate_flat(det_boxes, det_scores, det_labels, det_counts, gt_boxes, gt_labels, gt_counts, num_classes, iou_thrs=(0.25, 0.5),
                  device="cpu"):
    """Array-level entry: detections / GT concatenated over scenes (bottom-centre boxes [.,7], per-scene counts).
    -> dict with ap float32 [T, C], rec float64 [T, C], npos / ndet [C] (numpy) and the intermediate per-detection results."""
    det_boxes = np.asarray(to_numpy(det_boxes), np.float32).reshape(-1, 7)
    det_scores = np.asarray(to_numpy(det_scores), np.float32).reshape(-1)
    det_labels = np.asarray(to_numpy(det_labels), np.int64).reshape(-1)
    gt_boxes = np.asarray(to_numpy(gt_boxes), np.float32).reshape(-1, 7)
    gt_labels = np.asarray(to_numpy(gt_labels), np.int64).reshape(-1)
    det_off, gt_off = offsets(det_counts), offsets(gt_counts)
    _raise_invalid(invalid_host(det_scores, (det_labels, gt_labels)), None)
    num_classes = int(max(num_classes, det_labels.max(initial=-1) + 1, gt_labels.max(initial=-1) + 1))
    if torch.device(device).type == "cpu":
        return _host_eval(det_boxes, det_scores, det_labels, det_off, gt_boxes, gt_labels, gt_off, num_classes, iou_thrs)
    dev = torch.device(device)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)        # noqa: E731
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)      # noqa: E731
    return _device_eval(f32(det_boxes), f32(det_scores), i32(det_labels), i32(det_off), f32(gt_boxes), i32(gt_labels), i32(gt_off),
                        num_classes, iou_thrs, dev)


# --------------------------------------------------------------------------------------------------
# result dict and summary table
# --------------------------------------------------------------------------------------------------
def _nanmean(vals, dtype):
    v = np.asarray([x for x in vals if not np.isnan(x)], dtype)
    if v.size == 0:
        return float("nan")
    return float(np.mean(v))


def _results(res, label2cat, iou_thrs, logger):
    present = [c for c in range(len(res["npos"])) if res["npos"][c] > 0 or res["ndet"][c] > 0]
    ret = {}
    header = ["classes"]
    cols = [[str(label2cat[c]) for c in present] + ["Overall"]]
    for t, thr in enumerate(iou_thrs):
        header += [f"AP_{thr:.2f}", f"AR_{thr:.2f}"]
        aps = [res["ap"][t, c] for c in present]          # float32, averaged in float32 like the reference's np.mean
        for c, a in zip(present, aps):
            ret[f"{label2cat[c]}_AP_{thr:.2f}"] = float(a)
        ret[f"mAP_{thr:.2f}"] = _nanmean(aps, np.float32)
        recs = [float(res["rec"][t, c]) for c in present]
        for c, r in zip(present, recs):
            ret[f"{label2cat[c]}_rec_{thr:.2f}"] = r
        ret[f"mAR_{thr:.2f}"] = _nanmean(recs, np.float64)
        cols.append([f"{float(a):.4f}" for a in aps] + [f"{ret[f'mAP_{thr:.2f}']:.4f}"])
        cols.append([f"{r:.4f}" for r in recs] + [f"{ret[f'mAR_{thr:.2f}']:.4f}"])
    print_log("\n" + format_table([header] + [list(r) for r in zip(*cols)]), logger)
    return ret


def format_table(rows):
    """ASCII table with a rule under the header and above the last (footer) row."""
    w = [max(len(str(r[i])) for r in rows) for i in range(len(rows[0]))]
    rule = "+" + "+".join("-" * (x + 2) for x in w) + "+"
    line = lambda r: "| " + " | ".join(str(v).ljust(x) for v, x in zip(r, w)) + " |"      # noqa: E731
    out = [rule, line(rows[0]), rule] + [line(r) for r in rows[1:-1]] + ([rule, line(rows[-1])] if len(rows) > 1 else []) + [rule]
    return "\n".join(out)


# --------------------------------------------------------------------------------------------------
# public interface
# --------------------------------------------------------------------------------------------------
def indoor_eval(gt_annos, dt_annos, metric, label2cat, logger=None, box_type_3d=None, box_mode_3d=None, axis_aligned_lw=False, device=None):
    """mmdet3d's indoor_eval (the reference's indoor_eval_ov with every class seen): per-class AP / recall at each IoU threshold of
    `metric`, their means over the non-NaN classes, and a printed summary table.

    gt_annos: per scene {'gt_num', 'gt_boxes_upright_depth' (gravity-centre [n,6|7]), 'class'}; dt_annos: per scene {'boxes_3d',
    'scores_3d', 'labels_3d'} (tensors, arrays or box structures with `.tensor`), optionally under 'pts_bbox' (what
    `Uni3DETR.simple_test` returns).  Boxes are Depth-frame: box_type_3d / box_mode_3d are accepted for interface compatibility only.
    device: None = the GPU when there is one, else the host path; "cpu" forces the float64 host path."""
    assert len(dt_annos) == len(gt_annos)
    db, ds, dl, dc = _flatten_dt(dt_annos)
    gb, gl, gc = _flatten_gt(gt_annos, axis_aligned_lw)
    num_classes = int(max([int(k) for k in label2cat.keys()] + [-1])) + 1
    res = evaluate_flat(db, ds, dl, dc, gb, gl, gc, num_classes, tuple(metric), default_device(device))
    return _results(res, label2cat, tuple(metric), logger)


def indoor_eval_ov(seen_classes, gt_annos, dt_annos, metric, label2cat, logger=None, box_type_3d=None, box_mode_3d=None,
                   axis_aligned_lw=False, device=None):
    """The reference's signature: the same dict as `indoor_eval`, plus an informational line with the mean AP of the seen and of the
    unseen classes at the first threshold."""
    ret = indoor_eval(gt_annos, dt_annos, metric, label2cat, logger, box_type_3d, box_mode_3d, axis_aligned_lw, device)
    t = f"{metric[0]:.2f}"
    for name, keep in (("seen", True), ("unseen", False)):
        v = [ret[f"{cat}_AP_{t}"] for cat in label2cat.values() if (cat in seen_classes) == keep and f"{cat}_AP_{t}" in ret]
        if v:
            print_log(f"{name} AP{int(round(float(metric[0]) * 100))}: {_nanmean(v, np.float64)}", logger)
    return ret


class IndoorEvaluator:
    """Streaming indoor AP / recall over batches of `Uni3DETRHead.get_bboxes` output.

    add() appends whole batches to buffers on `device` (no host synchronisation); compute() runs the evaluation once over everything
    added.  The buffers are the concatenation of the scenes in the order they were added, so any batching of the same scenes gives
    bit-identical results."""

    def __init__(self, num_classes, iou_thrs=(0.25, 0.5), device="cuda"):
        self.num_classes = int(num_classes)
        self.iou_thrs = tuple(float(t) for t in iou_thrs)
        self.device = torch.device(device)
        self.reset()

    def reset(self):
        self._det = DetBuffer(7, torch.float32, self.device)
        self._gt = {"boxes": [], "labels": []}
        self._gt_counts = []

    def __len__(self):
        return len(self._det)

    def add(self, bbox_list, gt_boxes, gt_labels):
        """bbox_list: per scene [boxes [n,>=7] bottom-centre, scores [n], labels [n]] (or a dict with boxes_3d / scores_3d / labels_3d);
        gt_boxes: per scene a gravity-centre tensor [m,6|7] (gt_boxes_upright_depth layout), or a box structure with `.tensor`
        (bottom-centre, the mmdet3d convention of gt_bboxes_3d); gt_labels: per scene [m]."""
        assert len(bbox_list) == len(gt_boxes) == len(gt_labels)
        for det in bbox_list:
            self._det.add(det)                                              # a scene may have no detections
        self._add_gt(gt_boxes, gt_labels)

    def _add_gt(self, gt_boxes, gt_labels):
        dev = self.device
        for g, lab in zip(gt_boxes, gt_labels):
            gbox = fit_columns(as_tensor(g, torch.float32, dev), 7)
            if not hasattr(g, "tensor"):
                gbox = gbox.clone()
                gbox[:, 2] = gbox[:, 2] + gbox[:, 5] * -0.5                # gravity -> bottom centre, as _gt_bottom_boxes
            self._gt["boxes"].append(gbox)
            self._gt["labels"].append(as_tensor(lab, torch.int32, dev).reshape(-1))
            self._gt_counts.append(int(gbox.shape[0]))

    def add_store(self, store, gt_boxes, gt_labels):
        """add() for every scene of a det_store.DetStore at once, in the store's scene order: the detections are store.packed() (they
        never leave the device), the per-scene counts come from one read of its det_off.  gt_boxes / gt_labels: one entry per scene of
        the store, as for add().  Bit-identical to add() over the same scenes in the same order.  Labels are checked by compute()."""
        assert len(gt_boxes) == len(gt_labels)
        self._det.add_store(store, len(gt_boxes), f"IndoorEvaluator.add_store: the store holds {{n}} scenes, GT was given for {len(gt_boxes)}",
                            0, (ERRORS[0], ""))
        self._add_gt(gt_boxes, gt_labels)

    def compute(self, label2cat=None, logger="silent"):
        """-> the dict of `indoor_eval` (label2cat defaults to {c: str(c)}).  Labels outside [0, num_classes) raise ValueError."""
        if label2cat is None:
            label2cat = {c: str(c) for c in range(self.num_classes)}
        if not len(self):
            raise ValueError("IndoorEvaluator.compute: nothing was added")
        db, ds, dl, det_off = self._det.cat()
        gb = torch.cat(self._gt["boxes"]) if self._gt["boxes"] else torch.zeros((0, 7), dtype=torch.float32, device=self.device)
        gl = torch.cat(self._gt["labels"]) if self._gt["labels"] else torch.zeros((0,), dtype=torch.int32, device=self.device)
        if self.device.type == "cpu":
            _raise_invalid(invalid_host(ds.numpy(), (dl.numpy(), gl.numpy()), self.num_classes), self.num_classes)
            res = evaluate_flat(db, ds, dl, self._det.counts, gb, gl, self._gt_counts, self.num_classes, self.iou_thrs, "cpu")
        else:
            res = _device_eval(db, ds, dl, det_off, gb, gl, offsets(self._gt_counts, self.device), self.num_classes, self.iou_thrs, self.device)
        return _results(res, label2cat, self.iou_thrs, logger)
