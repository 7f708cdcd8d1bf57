"""nuScenes 3-D detection evaluation: per-class AP at four centre distances, the five TP errors, mAP and NDS (the `evaluation` of the
shipped nuScenes config, upstream `NuScenesSweepDataset.evaluate` -> `_format_bbox` -> the nuscenes-devkit's `NuScenesEval`).

Provenance: parity unpinned.  The devkit (and pyquaternion) is neither in the reference tree nor installed, so nothing here is pinned
against its source.  The semantics below are the contract, restated from the devkit's `detection_cvpr_2019` algorithm; the `ret_dict`
key names follow upstream `_evaluate_single` and are kept in `_KEYS` so a correction is one edit.

  * results are `Uni3DETR.simple_test` outputs (optionally under `pts_bbox`): LiDAR bottom-centre boxes [m, 9] (x, y, z, l, w, h, yaw
    counter-clockwise, vx, vy), scores, labels indexing `class_names`; infos are mmdet3d v1.0 nuScenes info dicts (token,
    lidar2ego_* / ego2global_* rotation (w, x, y, z) and translation, gt_boxes [g, 7] with the gravity centre, gt_names, gt_velocity,
    num_lidar_pts, num_radar_pts, and optionally gt_attr_names);
  * conversion, in float64: prediction centre z + h / 2, size wlh = (w, l, h), velocity (vx, vy, 0); each of lidar2ego and ego2global is
    the rotation matrix of its normalised quaternion followed by the translation; global yaw = atan2(R[1, 0], R[0, 0]) of the composed
    rotation; only the xy of the velocity is kept.  A prediction whose ego-frame xy radius is > class_range is dropped (upstream
    `lidar_nusc_box_to_global`).  GT rows are the info's gt_boxes whose gt_names is an evaluated class; gt_velocity (NaN allowed) is
    mapped back the same way.  A sample with more than 500 predictions raises ValueError (the devkit's max_boxes_per_sample assert,
    checked on the predictions handed in), as do non-finite scores and labels outside class_names;
  * prediction attribute (upstream `_format_bbox`): |v_xy| > 0.2 -> vehicle.moving (car, construction_vehicle, bus, truck, trailer),
    cycle.with_rider (bicycle, motorcycle), else the default; otherwise pedestrian.standing (pedestrian), vehicle.stopped (bus), else
    the default (DEFAULT_ATTRIBUTE); barrier and traffic_cone have '';
  * devkit filters on both sides: keep ego_dist < class_range (ego_dist = xy norm of the global centre minus ego2global_translation);
    drop GT with num_lidar_pts + num_radar_pts == 0; drop bicycle / motorcycle boxes whose centre lies inside (bounds inclusive, in
    the rack's own frame) one of the sample's `static_object.bicycle_rack` rows;
  * class_range: 50 m car / truck / bus / trailer / construction_vehicle, 40 m pedestrian / motorcycle / bicycle, 30 m traffic_cone /
    barrier; distance thresholds 0.5 / 1 / 2 / 4 m, TP threshold 2 m, min_recall = min_precision = 0.1, mean_ap_weight 5;
  * accumulate, per class and threshold: predictions ranked by sorted((score, global index))[::-1] (equal scores: the later (sample,
    position) first); each takes the untaken GT of its sample and class at minimum xy centre distance (strict '<', lowest GT index on
    ties) and is a TP iff that distance < the threshold; prec = tp / (tp + fp), rec = tp / npos interpolated with np.interp(
    linspace(0, 1, 101), rec, ., right=0) for precision and confidence; at 2 m the TP errors (centre distance, 1 - aligned wlh IoU,
    |angle_diff| with period pi for barrier and 2 pi otherwise, xy velocity L2, 1 - attribute equal / NaN for a GT attribute '') go
    through the NaN-aware cummean and np.interp at the confidences; npos == 0 or no TP gives no_predictions;
  * calc_ap = mean(max(prec[11:] - 0.1, 0)) / 0.9; calc_tp = mean over [11, max_recall_ind] (last non-zero confidence), 1.0 when
    empty; traffic_cone orient / vel / attr and barrier vel / attr are NaN; mAP = mean over classes of the mean over thresholds; each
    TP metric's mean is a nanmean over classes; NDS = (5 mAP + sum max(0, 1 - mTP)) / 10, with Python's max (a NaN mean scores 0).
  * GT attributes come from an optional per-box info['gt_attr_names'], which mmdet3d infos do not carry.  When no info has them, every
    attr_err and mAAE is NaN (a warning is logged) and NDS follows the devkit's arithmetic above (that term scores 0).

Two implementations of the same result: the device path (csrc/nusc_eval.hip through `native.nusc_to_global` / `native.nusc_metrics`;
ATen only scans the validity flags and stable-sorts the rank and segment keys) and a float64 NumPy restatement for `device="cpu"`,
which is the test yardstick.  Everything is deterministic: any batching of the same samples gives bit-identical results.
"""
import json
import logging
import math
import os
import warnings

import numpy as np
import torch

from .eval_common import DetBuffer, default_device, invalid_device, invalid_host, offsets, print_log, raise_invalid

# the messages of the prediction checks: a non-finite score, a label that does not index class_names; too few columns; too many boxes
ERRORS = ("nuscenes_eval: detection scores must be finite", "nuscenes_eval: labels must index class_names")
_SHORT = "nuscenes_eval: boxes_3d must have 9 columns (x, y, z, l, w, h, yaw, vx, vy)"
_TOO_MANY = "nuscenes_eval: a sample has {n} predictions, more than {cap}"
CLASSES = ("car", "truck", "trailer", "bus", "construction_vehicle", "bicycle", "motorcycle", "pedestrian", "traffic_cone", "barrier")
CLASS_RANGE = dict(car=50, truck=50, bus=50, trailer=50, construction_vehicle=50, pedestrian=40, motorcycle=40, bicycle=40,
                   traffic_cone=30, barrier=30)
DIST_THS = (0.5, 1.0, 2.0, 4.0)
DIST_TH_TP = 2.0
MIN_RECALL = 0.1
MIN_PRECISION = 0.1
MAX_BOXES_PER_SAMPLE = 500
MEAN_AP_WEIGHT = 5
TP_METRICS = ("trans_err", "scale_err", "orient_err", "vel_err", "attr_err")
ATTRIBUTES = ("cycle.with_rider", "cycle.without_rider", "pedestrian.moving", "pedestrian.standing", "pedestrian.sitting_lying_down",
              "vehicle.moving", "vehicle.parked", "vehicle.stopped")
DEFAULT_ATTRIBUTE = {"car": "vehicle.parked", "pedestrian": "pedestrian.moving", "trailer": "vehicle.parked", "truck": "vehicle.parked",
                     "bus": "vehicle.moving", "motorcycle": "cycle.without_rider", "construction_vehicle": "vehicle.parked",
                     "bicycle": "cycle.without_rider", "barrier": "", "traffic_cone": ""}
BIKE_RACK = "static_object.bicycle_rack"
DEFAULT_MODALITY = dict(use_camera=False, use_lidar=True, use_radar=False, use_map=False, use_external=False)
_REC_INTERP = np.linspace(0, 1, 101)
_TP_IDX = DIST_THS.index(DIST_TH_TP)
_OTHER, _RACK = -1, -2
# ret_dict naming (upstream _evaluate_single): prefix, per-class AP / TP error, the TP means, NDS / mAP
_KEYS = dict(prefix="{result_name}_NuScenes", ap="{p}/{cls}_AP_dist_{th}", tp="{p}/{cls}_{metric}", mean="{p}/{name}", nds="{p}/NDS",
             map="{p}/mAP", err_name={"trans_err": "mATE", "scale_err": "mASE", "orient_err": "mAOE", "vel_err": "mAVE",
                                      "attr_err": "mAAE"})
_log = logging.getLogger(__name__)


# --------------------------------------------------------------------------------------------------
# configuration tables
# --------------------------------------------------------------------------------------------------
def _attr_code(name):
    if name == "":
        return -1
    if name not in ATTRIBUTES:
        raise ValueError(f"nuscenes_eval: unknown attribute {name!r}")
    return ATTRIBUTES.index(name)


def _pred_attribute(name, moving):
    if moving:
        if name in ("car", "construction_vehicle", "bus", "truck", "trailer"):
            return "vehicle.moving"
        if name in ("bicycle", "motorcycle"):
            return "cycle.with_rider"
        return DEFAULT_ATTRIBUTE[name]
    if name == "pedestrian":
        return "pedestrian.standing"
    if name == "bus":
        return "vehicle.stopped"
    return DEFAULT_ATTRIBUTE[name]


class _Tables:
    """per-class constants of the evaluated classes (class_names order)"""

    def __init__(self, class_names):
        names = [str(c) for c in class_names]
        if not names or len(set(names)) != len(names) or any(c not in CLASSES for c in names):
            raise ValueError(f"nuscenes_eval: class_names must be distinct nuScenes detection classes {CLASSES}, got {tuple(names)}")
        self.names = names
        self.C = len(names)
        self.index = {c: i for i, c in enumerate(names)}
        self.range = np.asarray([CLASS_RANGE[c] for c in names], np.float64)
        self.attr_moving = np.asarray([_attr_code(_pred_attribute(c, True)) for c in names], np.int32)
        self.attr_still = np.asarray([_attr_code(_pred_attribute(c, False)) for c in names], np.int32)
        self.bike = np.asarray([c in ("bicycle", "motorcycle") for c in names], np.int32)
        self.period = np.asarray([np.pi if c == "barrier" else 2 * np.pi for c in names], np.float64)


def _check_version(eval_version):
    if eval_version != "detection_cvpr_2019":
        raise NotImplementedError(f"nuscenes_eval: only eval_version='detection_cvpr_2019' is implemented, got {eval_version!r}")


# --------------------------------------------------------------------------------------------------
# input encoding
# --------------------------------------------------------------------------------------------------
def quaternion_matrix(q):
    """rotation matrix [3, 3] of the quaternion (w, x, y, z), normalised first (float64)"""
    w, x, y, z = np.asarray(q, np.float64).reshape(4) / np.linalg.norm(np.asarray(q, np.float64).reshape(4))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _calib(info):
    """f64 [24] = lidar2ego rotation (row-major), translation, ego2global rotation, translation"""
    return np.concatenate([quaternion_matrix(info["lidar2ego_rotation"]).reshape(-1), np.asarray(info["lidar2ego_translation"], np.float64).reshape(3),
                           quaternion_matrix(info["ego2global_rotation"]).reshape(-1), np.asarray(info["ego2global_translation"], np.float64).reshape(3)])


def _pred_buffer(device, result_name="pts_bbox"):
    """predictions f64 [m, 9] with scores and labels; a sample with more than MAX_BOXES_PER_SAMPLE of them raises when it is added"""
    return DetBuffer(9, torch.float64, device, short=_SHORT, result_name=result_name, cap=MAX_BOXES_PER_SAMPLE, cap_message=_TOO_MANY)


def _host_arrays(buf, n_cls):
    """a host prediction buffer -> boxes f64 [m, 9], scores f64 [m], labels int64 [m], validated"""
    b, sc, lab, _ = (t.numpy() for t in buf.cat())
    raise_invalid(invalid_host(sc, lab, n_cls), ERRORS)
    return b, sc, lab


def _gt_arrays(info, tab):
    """-> rows f64 [g, 9] (x, y, z gravity, l, w, h, yaw, vx, vy), class int32 [g] (index, _OTHER, _RACK), points f64 [g], attribute
    code int32 [g], whether the info carries GT attributes"""
    names = [str(n) for n in np.asarray(info.get("gt_names", []), dtype=object).reshape(-1)]
    g = len(names)
    rows = np.zeros((g, 9))
    if g:
        rows[:, :7] = np.asarray(info["gt_boxes"], np.float64).reshape(g, -1)[:, :7]
        v = info.get("gt_velocity")
        rows[:, 7:9] = np.asarray(v, np.float64).reshape(g, 2) if v is not None else np.nan
    cls = np.asarray([tab.index.get(n, _RACK if n == BIKE_RACK else _OTHER) for n in names], np.int32)
    pts = np.zeros(g)
    for k in ("num_lidar_pts", "num_radar_pts"):
        if k in info:
            pts = pts + np.asarray(info[k], np.float64).reshape(g)
    has_attr = "gt_attr_names" in info
    attrs = [str(a) for a in np.asarray(info["gt_attr_names"], dtype=object).reshape(-1)] if has_attr else [""] * g
    attr = np.asarray([_attr_code(a) for a in attrs], np.int32).reshape(g)
    return rows, cls, pts, attr, has_attr


# --------------------------------------------------------------------------------------------------
# host path (float64 NumPy)
# --------------------------------------------------------------------------------------------------
def _rot(R, x, y, z):
    return R[0] * x + R[1] * y + R[2] * z, R[3] * x + R[4] * y + R[5] * z, R[6] * x + R[7] * y + R[8] * z


def to_global(rows, cls, aux, attr, counts, calib, is_pred, tab):
    """float64 restatement of u3d_nusc_convert: LiDAR rows [n, 9] -> (records [n, 12], valid bool [n]); calib [S, 24] per sample."""
    n = rows.shape[0]
    s_of = np.repeat(np.arange(len(counts)), counts)
    K = calib[s_of].T if n else np.zeros((24, 0))
    R1, t1, R2, t2 = K[0:9], K[9:12], K[12:21], K[21:24]
    x, y, l, w, h, yaw, vx, vy = rows[:, 0], rows[:, 1], rows[:, 3], rows[:, 4], rows[:, 5], rows[:, 6], rows[:, 7], rows[:, 8]
    z = rows[:, 2] + h / 2.0 if is_pred else rows[:, 2]
    ex, ey, ez = _rot(R1, x, y, z)
    ex, ey, ez = ex + t1[0], ey + t1[1], ez + t1[2]
    gx, gy, gz = _rot(R2, ex, ey, ez)
    gx, gy, gz = gx + t2[0], gy + t2[1], gz + t2[2]
    c, sn = np.cos(yaw), np.sin(yaw)
    u0, u1, u2 = R1[0] * c + R1[1] * sn, R1[3] * c + R1[4] * sn, R1[6] * c + R1[7] * sn
    gyaw = np.arctan2(R2[3] * u0 + R2[4] * u1 + R2[5] * u2, R2[0] * u0 + R2[1] * u1 + R2[2] * u2)
    a0, a1, a2 = R1[0] * vx + R1[1] * vy, R1[3] * vx + R1[4] * vy, R1[6] * vx + R1[7] * vy
    gvx, gvy = R2[0] * a0 + R2[1] * a1 + R2[2] * a2, R2[3] * a0 + R2[4] * a1 + R2[5] * a2
    cls = np.asarray(cls, np.int64)
    known = (cls >= 0) & (cls < tab.C)
    cc = np.where(known, cls, 0)
    if is_pred:
        valid = known & ~(np.sqrt(ex * ex + ey * ey) > tab.range[cc])
        moving = np.sqrt(gvx * gvx + gvy * gvy) > 0.2
        a11 = np.where(valid, np.where(moving, tab.attr_moving[cc], tab.attr_still[cc]), -1).astype(np.float64)
    else:
        valid = known | (cls == _RACK)
        a11 = np.where(cls == _RACK, yaw, np.asarray(attr, np.float64))
    rec = np.stack([gx, gy, gz, w, l, h, gyaw, gvx, gvy, np.asarray(aux, np.float64), np.where(known | (cls == _RACK), cls, _OTHER), a11], 1)
    return rec.reshape(n, 12), valid


def _in_rack(p, rk, R1, R2):
    d0, d1, d2 = p[:, 0] - rk[0], p[:, 1] - rk[1], p[:, 2] - rk[2]
    a0, a1, a2 = R2[0] * d0 + R2[3] * d1 + R2[6] * d2, R2[1] * d0 + R2[4] * d1 + R2[7] * d2, R2[2] * d0 + R2[5] * d1 + R2[8] * d2
    b0, b1, b2 = R1[0] * a0 + R1[3] * a1 + R1[6] * a2, R1[1] * a0 + R1[4] * a1 + R1[7] * a2, R1[2] * a0 + R1[5] * a1 + R1[8] * a2
    c, sn = np.cos(rk[11]), np.sin(rk[11])
    lx, ly = c * b0 + sn * b1, c * b1 - sn * b0
    return (np.abs(lx) <= rk[4] / 2.0) & (np.abs(ly) <= rk[3] / 2.0) & (np.abs(b2) <= rk[5] / 2.0)


def devkit_filter(rec, valid, counts, calib, gt_rec, gt_counts, is_pred, tab):
    """float64 restatement of u3d_nusc_filter -> valid bool [n]"""
    valid = valid.copy()
    off, goff = offsets(counts), offsets(gt_counts)
    for s in range(len(counts)):
        r = rec[off[s]:off[s + 1]]
        v = valid[off[s]:off[s + 1]]
        k = r[:, 10].astype(np.int64)
        known = (k >= 0) & (k < tab.C)
        kc = np.where(known, k, 0)
        dx, dy = r[:, 0] - calib[s, 21], r[:, 1] - calib[s, 22]
        v &= known & (np.sqrt(dx * dx + dy * dy) < tab.range[kc])
        if not is_pred:
            v &= r[:, 9] != 0.0
        g = gt_rec[goff[s]:goff[s + 1]]
        racks = g[g[:, 10] == _RACK]
        bike = v & (tab.bike[kc] == 1)
        for rk in racks:
            if bike.any():
                v &= ~(bike & _in_rack(r, rk, calib[s, 0:9], calib[s, 12:21]))
        valid[off[s]:off[s + 1]] = v
    return valid


def _compact(rec, valid, counts):
    off = offsets(counts)
    return rec[valid], [int(valid[off[s]:off[s + 1]].sum()) for s in range(len(counts))]


def host_match(pred, pred_counts, gt, gt_counts, tab):
    """greedy matching of every (class, threshold) -> rank int64 [n] (prediction rows in rank order), cseg [C+1], tp int8 [4, n] and
    match int64 [n] (GT row at 2 m, -1 = none) by rank position, npos [C]."""
    S = len(pred_counts)
    ps = np.repeat(np.arange(S), pred_counts)
    gs = np.repeat(np.arange(S), gt_counts)
    pc, gc = pred[:, 10].astype(np.int64), gt[:, 10].astype(np.int64)
    n = pred.shape[0]
    rank, cseg = [], [0]
    tp = np.zeros((len(DIST_THS), n), np.int8)
    match = np.full(n, -1, np.int64)
    for c in range(tab.C):
        rows = np.nonzero(pc == c)[0]
        order = rows[np.lexsort((rows, pred[rows, 9]))[::-1]]         # sorted((score, index))[::-1]
        base = len(rank)
        rank.extend(order.tolist())
        cseg.append(len(rank))
        gt_of = {s: np.nonzero((gs == s) & (gc == c))[0] for s in np.unique(ps[order])}
        taken = {s: np.zeros((len(DIST_THS), len(g)), bool) for s, g in gt_of.items()}
        for k, i in enumerate(order):
            s = ps[i]
            g = gt_of[s]
            if not len(g):
                continue
            dx, dy = pred[i, 0] - gt[g, 0], pred[i, 1] - gt[g, 1]
            dist = np.sqrt(dx * dx + dy * dy)
            for t, th in enumerate(DIST_THS):
                dm = np.where(taken[s][t], np.inf, dist)
                j = int(np.argmin(dm))                                  # the first minimum: the lowest GT index on ties
                if dm[j] < th:
                    taken[s][t, j] = True
                    tp[t, base + k] = 1
                    if t == _TP_IDX:
                        match[base + k] = g[j]
    npos = np.bincount(gc, minlength=tab.C)[:tab.C] if gt.shape[0] else np.zeros(tab.C, np.int64)
    return np.asarray(rank, np.int64), np.asarray(cseg, np.int64), tp, match, npos


def cummean(x):
    """the devkit's NaN-aware cumulative mean (all NaN -> ones)"""
    if np.sum(np.isnan(x)) == len(x):
        return np.ones(len(x))
    sum_vals = np.nancumsum(x.astype(float))
    count_vals = np.cumsum(~np.isnan(x))
    return np.divide(sum_vals, count_vals, out=np.zeros_like(sum_vals), where=count_vals != 0)


def angle_diff(x, y, period):
    diff = (x - y + period / 2) % period - period / 2
    return np.where(diff > np.pi, diff - 2 * np.pi, diff)


def tp_errors(p, g, period):
    """[5, k] errors of matched (prediction, GT) record pairs: trans, scale, orient, vel, attr"""
    dx, dy = p[:, 0] - g[:, 0], p[:, 1] - g[:, 1]
    dvx, dvy = p[:, 7] - g[:, 7], p[:, 8] - g[:, 8]
    inter = np.minimum(g[:, 3], p[:, 3]) * np.minimum(g[:, 4], p[:, 4]) * np.minimum(g[:, 5], p[:, 5])
    va, vr = g[:, 3] * g[:, 4] * g[:, 5], p[:, 3] * p[:, 4] * p[:, 5]
    attr = np.where(g[:, 11] < 0, np.nan, 1.0 - (g[:, 11] == p[:, 11]).astype(np.float64))
    return np.stack([np.sqrt(dx * dx + dy * dy), 1.0 - inter / (va + vr - inter), np.abs(angle_diff(g[:, 6], p[:, 6], period)),
                     np.sqrt(dvx * dvx + dvy * dvy), attr])


def metric_data(tp, conf, npos, errs=None, match_conf=None):
    """the devkit's accumulate after matching, for one (class, threshold): tp [n] and conf [n] in rank order; errs [5, T] / match_conf
    [T] of the TPs (None: no TP errors).  -> dict(prec, conf, err [5, 101] | None, max_recall_ind, no_pred)."""
    n_tp = int(np.sum(tp))
    if npos == 0 or n_tp == 0:
        return dict(prec=np.zeros(101), conf=np.zeros(101), err=np.ones((5, 101)), max_recall_ind=0, no_pred=True)
    tpc = np.cumsum(tp).astype(float)
    fpc = np.cumsum(1 - np.asarray(tp, np.int64)).astype(float)
    prec = tpc / (fpc + tpc)
    rec = tpc / float(npos)
    prec = np.interp(_REC_INTERP, rec, prec, right=0)
    conf = np.interp(_REC_INTERP, rec, conf, right=0)
    err = None
    if errs is not None:
        err = np.stack([np.interp(conf[::-1], match_conf[::-1], cummean(e)[::-1])[::-1] for e in errs])
    nz = np.nonzero(conf)[0]
    return dict(prec=prec, conf=conf, err=err, max_recall_ind=int(nz[-1]) if len(nz) else 0, no_pred=False)


def calc_ap(prec):
    p = np.copy(prec)[round(100 * MIN_RECALL) + 1:] - MIN_PRECISION
    p[p < 0] = 0
    return float(np.mean(p)) / (1.0 - MIN_PRECISION)


def calc_tp(err, max_recall_ind):
    first = round(100 * MIN_RECALL) + 1
    if max_recall_ind < first:
        return 1.0
    return float(np.mean(err[first:max_recall_ind + 1]))


def host_metrics(pred, gt, rank, cseg, tp, match, npos, tab):
    """float64 restatement of u3d_nusc_accumulate -> dict(ap [C, 4], tp_err [C, 5], prec / conf [C, 4, 101], err [C, 5, 101], mri)."""
    C = tab.C
    ap, tp_err = np.zeros((C, len(DIST_THS))), np.ones((C, 5))
    prec, conf = np.zeros((C, len(DIST_THS), 101)), np.zeros((C, len(DIST_THS), 101))
    err, mri = np.ones((C, 5, 101)), np.zeros((C, len(DIST_THS)), np.int64)
    for c in range(C):
        r = rank[cseg[c]:cseg[c + 1]]
        sc = pred[r, 9]
        for t in range(len(DIST_THS)):
            f = tp[t, cseg[c]:cseg[c + 1]].astype(np.int64)
            errs = mc = None
            if t == _TP_IDX and f.any():
                hit = np.nonzero(f)[0]
                errs = tp_errors(pred[r[hit]], gt[match[cseg[c] + hit]], tab.period[c])
                mc = sc[hit]
            md = metric_data(f, sc, int(npos[c]), errs, mc)
            prec[c, t], conf[c, t], mri[c, t] = md["prec"], md["conf"], md["max_recall_ind"]
            ap[c, t] = calc_ap(md["prec"])
            if t == _TP_IDX:
                err[c] = md["err"]
                tp_err[c] = [calc_tp(e, md["max_recall_ind"]) for e in md["err"]]
    return dict(ap=ap, tp_err=tp_err, prec=prec, conf=conf, err=err, mri=mri)


class _Encoded:
    """(results, infos) as the evaluation takes them: the predictions in a DetBuffer on `device`, and the host encoding of the infos -
    LiDAR rows, classes, points, attributes and counts of the GT, calibration"""

    def __init__(self, tab, device="cpu", result_name="pts_bbox"):
        self.tab = tab
        self.pred = _pred_buffer(device, result_name)
        self.g_rows, self.g_cls, self.g_pts, self.g_attr, self.g_counts = [], [], [], [], []
        self.g_dev, self.calib, self.tokens, self.has_attr = [], [], [], []

    def add_gt(self, info):
        rows, cls, pts, attr, has = _gt_arrays(info, self.tab)
        self.g_rows.append(rows)
        self.g_cls.append(cls)
        self.g_pts.append(pts)
        self.g_attr.append(attr)
        self.g_counts.append(rows.shape[0])
        self.g_dev.append(tuple(torch.as_tensor(x, device=self.pred.device) for x in (rows, cls, pts, attr)))
        self.calib.append(_calib(info))
        self.tokens.append(info.get("token", str(len(self.tokens))))
        self.has_attr.append(has)

    def add_pred(self, res):
        self.pred.add(res)

    @staticmethod
    def _cat(xs, shape, dtype):
        return np.concatenate(xs).astype(dtype) if xs else np.zeros(shape, dtype)

    def arrays(self):
        """everything on the host (a host buffer), the predictions validated"""
        b, sc, lab = _host_arrays(self.pred, self.tab.C)
        return dict(p_rows=b, p_score=sc, p_lab=lab.astype(np.int32), p_counts=list(self.pred.counts),
                    g_rows=self._cat(self.g_rows, (0, 9), np.float64), g_cls=self._cat(self.g_cls, (0,), np.int32),
                    g_pts=self._cat(self.g_pts, (0,), np.float64), g_attr=self._cat(self.g_attr, (0,), np.int32),
                    g_counts=list(self.g_counts), calib=np.asarray(self.calib, np.float64).reshape(-1, 24))

    def gt_device(self):
        """the GT as device_global takes it: what add_gt left on the buffer's device, concatenated"""
        dev = self.pred.device
        g_rows, g_cls, g_pts, g_attr = (torch.cat([g[k] for g in self.g_dev]).contiguous() for k in range(4))
        return dict(g_rows=g_rows.reshape(-1, 9), g_cls=g_cls, g_pts=g_pts, g_attr=g_attr, g_off=offsets(self.g_counts, dev),
                    calib=torch.as_tensor(np.asarray(self.calib, np.float64).reshape(-1, 24), device=dev))


def host_global(a, tab):
    """encoded arrays -> filtered global records (pred, pred counts, gt, gt counts)"""
    grec, gval = to_global(a["g_rows"], a["g_cls"], a["g_pts"], a["g_attr"], a["g_counts"], a["calib"], False, tab)
    gval = devkit_filter(grec, gval, a["g_counts"], a["calib"], grec, a["g_counts"], False, tab)
    prec_, pval = to_global(a["p_rows"], a["p_lab"], a["p_score"], None, a["p_counts"], a["calib"], True, tab)
    pval = devkit_filter(prec_, pval, a["p_counts"], a["calib"], grec, a["g_counts"], True, tab)
    pred, pc = _compact(prec_, pval, a["p_counts"])
    gt, gc = _compact(grec, gval, a["g_counts"])
    return pred, pc, gt, gc


def host_core(pred, pred_counts, gt, gt_counts, tab):
    """float64 path over filtered global records -> dict(ap, tp_err, rank, cseg, tp, match, npos, prec, conf, err, mri)"""
    rank, cseg, tp, match, npos = host_match(pred, pred_counts, gt, gt_counts, tab)
    out = host_metrics(pred, gt, rank, cseg, tp, match, npos, tab)
    out.update(rank=rank, cseg=cseg, tp=tp, match=match, npos=npos)
    return out


# --------------------------------------------------------------------------------------------------
# device path
# --------------------------------------------------------------------------------------------------
def _dev_tables(tab, dev):
    f64 = lambda a: torch.as_tensor(np.asarray(a, np.float64), device=dev)   # noqa: E731
    i32 = lambda a: torch.as_tensor(np.asarray(a, np.int32), device=dev)     # noqa: E731
    return dict(range=f64(tab.range), moving=i32(tab.attr_moving), still=i32(tab.attr_still), bike=i32(tab.bike), period=f64(tab.period),
                ths=f64(DIST_THS), ri=f64(_REC_INTERP))


def device_global(p_rows, p_score, p_lab, p_off, g_rows, g_cls, g_pts, g_attr, g_off, calib, dt):
    """device tensors (rows f64, labels / classes / attributes int32, offsets int32 [S+1], calib f64 [S, 24]) -> (pred records,
    offsets, GT records, offsets) after conversion, filters and compaction"""
    from . import native as nv
    graw, gval, gt, gt_off = nv.nusc_to_global(g_rows, g_cls, g_attr, g_pts, g_off, calib, False, dt["range"], dt["moving"], dt["still"],
                                               dt["bike"])
    _, _, pred, pred_off = nv.nusc_to_global(p_rows, p_lab, None, p_score, p_off, calib, True, dt["range"], dt["moving"], dt["still"],
                                             dt["bike"], gt_rec=graw, gt_off=g_off)
    return pred, pred_off, gt, gt_off


def device_core(pred, pred_off, gt, gt_off, tab, dt):
    """device path over filtered global records (f64 [., 12] with offsets int32 [S+1]) -> dict of host numpy arrays (as host_core)"""
    from . import native as nv
    r = nv.nusc_metrics(pred, pred_off, gt, gt_off, tab.C, dt["ths"], _TP_IDX, dt["ri"], dt["period"])
    return {k: v.cpu().numpy() for k, v in r.items()}


def _upload_encoded(a, dev):
    f64 = lambda x: torch.as_tensor(x, dtype=torch.float64, device=dev).contiguous()   # noqa: E731
    i32 = lambda x: torch.as_tensor(x, dtype=torch.int32, device=dev).contiguous()     # noqa: E731
    return dict(p_rows=f64(a["p_rows"]), p_score=f64(a["p_score"]), p_lab=i32(a["p_lab"]), p_off=offsets(a["p_counts"], dev),
                g_rows=f64(a["g_rows"]), g_cls=i32(a["g_cls"]), g_pts=f64(a["g_pts"]), g_attr=i32(a["g_attr"]), g_off=offsets(a["g_counts"], dev),
                calib=f64(a["calib"]))


# --------------------------------------------------------------------------------------------------
# results
# --------------------------------------------------------------------------------------------------
def _round4(v):
    return float("{:.4f}".format(v))


def summarize(ap, tp_err, class_names, attr_known=True):
    """per-class AP [C, 4] and calc_tp [C, 5] -> (label_aps, label_tp_errors, mean_ap, tp_errors, nd_score), the devkit's
    DetectionMetrics (class NaNs applied)."""
    label_aps = {c: {th: float(ap[i, t]) for t, th in enumerate(DIST_THS)} for i, c in enumerate(class_names)}
    label_tp = {}
    for i, c in enumerate(class_names):
        d = {}
        for m, name in enumerate(TP_METRICS):
            if c == "traffic_cone" and name in ("attr_err", "vel_err", "orient_err"):
                v = np.nan
            elif c == "barrier" and name in ("attr_err", "vel_err"):
                v = np.nan
            elif name == "attr_err" and not attr_known:
                v = np.nan
            else:
                v = float(tp_err[i, m])
            d[name] = v
        label_tp[c] = d
    mean_ap = float(np.mean([np.mean(list(d.values())) for d in label_aps.values()]))
    tp_errors = {}
    for name in TP_METRICS:
        vals = np.asarray([label_tp[c][name] for c in class_names], np.float64)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            tp_errors[name] = float(np.nanmean(vals))
    tp_scores = {name: max(0.0, 1.0 - tp_errors[name]) for name in TP_METRICS}
    nds = float(MEAN_AP_WEIGHT * mean_ap + np.sum(list(tp_scores.values()))) / float(MEAN_AP_WEIGHT + len(tp_scores))
    return label_aps, label_tp, mean_ap, tp_errors, nds


def _results(ap, tp_err, class_names, result_name="pts_bbox", attr_known=True, logger=None):
    label_aps, label_tp, mean_ap, tp_errors, nds = summarize(ap, tp_err, class_names, attr_known)
    p = _KEYS["prefix"].format(result_name=result_name)
    ret = {}
    for c in class_names:
        for th, v in label_aps[c].items():
            ret[_KEYS["ap"].format(p=p, cls=c, th=th)] = _round4(v)
        for m, v in label_tp[c].items():
            ret[_KEYS["tp"].format(p=p, cls=c, metric=m)] = _round4(v)
        for m, v in tp_errors.items():
            ret[_KEYS["mean"].format(p=p, name=_KEYS["err_name"][m])] = _round4(v)
    ret[_KEYS["nds"].format(p=p)] = nds
    ret[_KEYS["map"].format(p=p)] = mean_ap
    if logger != "silent":
        lines = [f"mAP: {mean_ap:.4f}"] + [f"{_KEYS['err_name'][m]}: {v:.4f}" for m, v in tp_errors.items()] + [f"NDS: {nds:.4f}", "",
                                                                                                                 "Per-class results:"]
        lines.append(f"{'Object Class':<22}{'AP':>8}{'ATE':>8}{'ASE':>8}{'AOE':>8}{'AVE':>8}{'AAE':>8}")
        for c in class_names:
            e = label_tp[c]
            lines.append(f"{c:<22}{np.mean(list(label_aps[c].values())):8.3f}" + "".join(f"{e[m]:8.3f}" for m in TP_METRICS))
        print_log("\n" + "\n".join(lines), logger)
    return ret


def _attr_warning(attr_known, logger):
    if not attr_known:
        msg = "nuscenes_eval: the infos carry no gt_attr_names: every attr_err and mAAE is NaN (the NDS term scores 0)"
        if isinstance(logger, logging.Logger):
            logger.warning(msg)
        else:
            _log.warning(msg)


def evaluate_encoded(a, tab, device="cpu"):
    """encoded arrays (_Encoded.arrays()) -> dict with ap [C, 4], tp_err [C, 5] and the intermediate arrays (numpy)"""
    dev = torch.device(device)
    if dev.type == "cpu":
        pred, pc, gt, gc = host_global(a, tab)
        return host_core(pred, pc, gt, gc, tab)
    dt = _dev_tables(tab, dev)
    u = _upload_encoded(a, dev)
    pred, pred_off, gt, gt_off = device_global(u["p_rows"], u["p_score"], u["p_lab"], u["p_off"], u["g_rows"], u["g_cls"], u["g_pts"],
                                               u["g_attr"], u["g_off"], u["calib"], dt)
    return device_core(pred, pred_off, gt, gt_off, tab, dt)


def nuscenes_eval(results, infos, class_names=CLASSES, eval_version="detection_cvpr_2019", result_name="pts_bbox", logger=None, device=None):
    """The devkit's detection evaluation of `simple_test` results -> upstream `_evaluate_single`'s ret_dict.
    device: None = the GPU when there is one, "cpu" = the float64 host path."""
    _check_version(eval_version)
    if len(results) != len(infos):
        raise ValueError("nuscenes_eval: one result per info")
    tab = _Tables(class_names)
    enc = _Encoded(tab, result_name=result_name)
    for res, info in zip(results, infos):
        enc.add_gt(info)
        enc.add_pred(res)
    attr_known = any(enc.has_attr)
    _attr_warning(attr_known, logger)
    r = evaluate_encoded(enc.arrays(), tab, default_device(device))
    return _results(r["ap"], r["tp_err"], tab.names, result_name, attr_known, logger)


# --------------------------------------------------------------------------------------------------
# LiDAR results -> the devkit's submission format (host only)
# --------------------------------------------------------------------------------------------------
def _qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                      w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def lidar_results_to_nusc(results, infos, class_names=CLASSES, modality=None):
    """`simple_test` results -> the devkit submission dict {'meta', 'results': {token: [box dicts]}} (upstream `_format_bbox`: the
    ego-radius drop only; the devkit applies its own filters)."""
    if len(results) != len(infos):
        raise ValueError("nuscenes_eval: one result per info")
    tab = _Tables(class_names)
    out = {}
    for res, info in zip(results, infos):
        buf = _pred_buffer("cpu")
        buf.add(res)
        b, sc, lab = _host_arrays(buf, tab.C)
        cal = _calib(info)[None]
        rec, valid = to_global(b, lab.astype(np.int32), sc, None, [b.shape[0]], cal, True, tab)
        q = _qmul(np.asarray(info["ego2global_rotation"], np.float64) / np.linalg.norm(info["ego2global_rotation"]),
                  np.asarray(info["lidar2ego_rotation"], np.float64) / np.linalg.norm(info["lidar2ego_rotation"]))
        annos = []
        for i in np.nonzero(valid)[0]:
            yaw = b[i, 6]
            qi = _qmul(q, np.array([math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2)]))
            name = tab.names[int(lab[i])]
            a = int(rec[i, 11])
            annos.append(dict(sample_token=info["token"], translation=rec[i, 0:3].tolist(), size=rec[i, 3:6].tolist(),
                              rotation=(qi / np.linalg.norm(qi)).tolist(), velocity=rec[i, 7:9].tolist(), detection_name=name,
                              detection_score=float(sc[i]), attribute_name=ATTRIBUTES[a] if a >= 0 else ""))
        out[info["token"]] = annos
    return {"meta": dict(DEFAULT_MODALITY if modality is None else modality), "results": out}


def format_results(results, infos, jsonfile_prefix, class_names=CLASSES, modality=None):
    """write `{jsonfile_prefix}/results_nusc.json` (the devkit submission) -> its path"""
    os.makedirs(jsonfile_prefix, exist_ok=True)
    path = os.path.join(jsonfile_prefix, "results_nusc.json")
    with open(path, "w") as f:
        json.dump(lidar_results_to_nusc(results, infos, class_names, modality), f)
    return path


class NuScenesEvaluator:
    """Streaming nuScenes evaluation over `simple_test` batches.

    add(results, infos) keeps the predictions on `device` (boxes, scores, labels; a sample with more than 500 predictions raises at once)
    and encodes the GT of `infos` once (LiDAR rows, classes, points, attributes, calibration), uploading it to the device.  compute()
    converts, filters, matches and accumulates everything added in one pass, so any batching of the same samples gives bit-identical
    results."""

    def __init__(self, class_names=CLASSES, device="cuda", eval_version="detection_cvpr_2019", result_name="pts_bbox"):
        _check_version(eval_version)
        self.tab = _Tables(class_names)
        self.class_names = self.tab.names
        self.device = torch.device(device)
        self.result_name = result_name
        self.reset()

    def reset(self):
        self._enc = _Encoded(self.tab, self.device, self.result_name)

    def __len__(self):
        return len(self._enc.g_counts)

    def add(self, results, infos):
        if len(results) != len(infos):
            raise ValueError("nuscenes_eval: one result per info")
        for res, info in zip(results, infos):
            self._enc.add_pred(res)
            self._enc.add_gt(info)

    def add_store(self, store, infos):
        """add() for every sample of a det_store.DetStore (box_dim 9) at once, in the store's scene order: the predictions are
        store.packed() (they never leave the device, float32 -> float64 there is exact), the per-sample counts come from one read of
        its det_off.  Bit-identical to add() over the same samples in the same order."""
        self._enc.pred.add_store(store, len(infos), "nuscenes_eval: one result per info", self.tab.C, ERRORS)
        for info in infos:
            self._enc.add_gt(info)

    def compute(self, logger="silent"):
        """-> ret_dict of `nuscenes_eval` over everything added (the summary goes to `logger`)."""
        if not len(self):
            raise ValueError("NuScenesEvaluator.compute: nothing was added")
        attr_known = any(self._enc.has_attr)
        _attr_warning(attr_known, logger)
        if self.device.type == "cpu":
            r = evaluate_encoded(self._enc.arrays(), self.tab, "cpu")
            return _results(r["ap"], r["tp_err"], self.class_names, self.result_name, attr_known, logger)
        boxes, scores, labels, p_off = self._enc.pred.cat()
        raise_invalid(invalid_device(scores, labels, self.tab.C), ERRORS)
        u = self._enc.gt_device()
        dt = _dev_tables(self.tab, self.device)
        pred, pred_off, gt, gt_off = device_global(boxes, scores, labels, p_off, u["g_rows"], u["g_cls"], u["g_pts"], u["g_attr"], u["g_off"],
                                                   u["calib"], dt)
        r = device_core(pred, pred_off, gt, gt_off, self.tab, dt)
        return _results(r["ap"], r["tp_err"], self.class_names, self.result_name, attr_known, logger)
