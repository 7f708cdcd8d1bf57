"""A literal, loop-by-loop restatement of the nuScenes detection evaluation (upstream `_format_bbox` + the devkit's detection_cvpr_2019
load / filter / accumulate / calc_ap / calc_tp / DetectionMetrics), written from the algorithm and deliberately independent of
uni3detr_amd/nuscenes_eval.py: quaternion algebra instead of rotation matrices, dicts of boxes, one Python loop per box, the devkit's
corner-based points_in_box, and np.interp / cummean applied as the devkit writes them."""
import math

import numpy as np

CLASSES = ("car", "truck", "trailer", "bus", "construction_vehicle", "bicycle", "motorcycle", "pedestrian", "traffic_cone", "barrier")
CLASS_RANGE = {"car": 50, "truck": 50, "bus": 50, "trailer": 50, "construction_vehicle": 50, "pedestrian": 40, "motorcycle": 40,
               "bicycle": 40, "traffic_cone": 30, "barrier": 30}
DIST_THS = [0.5, 1.0, 2.0, 4.0]
DIST_TH_TP = 2.0
MIN_RECALL, MIN_PRECISION, MEAN_AP_WEIGHT = 0.1, 0.1, 5
TP_METRICS = ["trans_err", "scale_err", "orient_err", "vel_err", "attr_err"]
DEFAULT_ATTRIBUTE = {"car": "vehicle.parked", "pedestrian": "pedestrian.moving", "trailer": "vehicle.parked", "truck": "vehicle.parked",
                     "bus": "vehicle.moving", "motorcycle": "cycle.without_rider", "construction_vehicle": "vehicle.parked",
                     "bicycle": "cycle.without_rider", "barrier": "", "traffic_cone": ""}


# ---------------------------------------------------------------- quaternions (w, x, y, z)
def q_normalise(q):
    n = math.sqrt(sum(float(c) * float(c) for c in q))
    return [float(c) / n for c in q]


def q_mul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return [w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
            w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2]


def q_rotate(q, v):
    r = q_mul(q_mul(q, [0.0, v[0], v[1], v[2]]), [q[0], -q[1], -q[2], -q[3]])
    return [r[1], r[2], r[3]]


def q_yaw(yaw):
    return [math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2)]


def quaternion_yaw(q):
    v = q_rotate(q, [1.0, 0.0, 0.0])
    return math.atan2(v[1], v[0])


# ---------------------------------------------------------------- boxes
def _box(center, wlh, yaw, velocity):
    return dict(center=[float(c) for c in center], wlh=[float(c) for c in wlh], q=q_yaw(float(yaw)),
                velocity=[float(velocity[0]), float(velocity[1]), 0.0])


def _rotate(box, q):
    box["center"] = q_rotate(q, box["center"])
    box["q"] = q_mul(q, box["q"])
    box["velocity"] = q_rotate(q, box["velocity"])


def _translate(box, t):
    box["center"] = [box["center"][k] + float(t[k]) for k in range(3)]


def attribute(name, velocity):
    if np.sqrt(velocity[0] ** 2 + velocity[1] ** 2) > 0.2:
        if name in ["car", "construction_vehicle", "bus", "truck", "trailer"]:
            return "vehicle.moving"
        if name in ["bicycle", "motorcycle"]:
            return "cycle.with_rider"
        return DEFAULT_ATTRIBUTE[name]
    if name in ["pedestrian"]:
        return "pedestrian.standing"
    if name in ["bus"]:
        return "vehicle.stopped"
    return DEFAULT_ATTRIBUTE[name]


def _to_global(box, info):
    _rotate(box, q_normalise(info["lidar2ego_rotation"]))
    _translate(box, info["lidar2ego_translation"])
    radius = np.linalg.norm(box["center"][:2], 2)
    _rotate(box, q_normalise(info["ego2global_rotation"]))
    _translate(box, info["ego2global_translation"])
    return radius


def format_results(results, infos, class_names=CLASSES):
    """-> {token: [EvalBox dicts]} of the predictions (upstream output_to_nusc_box + lidar_nusc_box_to_global + _format_bbox)"""
    out = {}
    for res, info in zip(results, infos):
        res = res.get("pts_bbox", res)
        boxes = np.asarray(res["boxes_3d"], np.float64).reshape(-1, 9)
        scores = np.asarray(res["scores_3d"], np.float64).reshape(-1)
        labels = np.asarray(res["labels_3d"]).reshape(-1)
        annos = []
        for i in range(boxes.shape[0]):
            x, y, z, l, w, h, yaw, vx, vy = boxes[i]
            name = class_names[int(labels[i])]
            box = _box([x, y, z + h / 2], [w, l, h], yaw, [vx, vy])
            if _to_global(box, info) > CLASS_RANGE[name]:
                continue
            annos.append(dict(sample_token=info["token"], translation=box["center"], size=box["wlh"], rotation=box["q"],
                              velocity=box["velocity"][:2], detection_name=name, detection_score=float(scores[i]),
                              attribute_name=attribute(name, box["velocity"]), num_pts=-1))
        out[info["token"]] = annos
    return out


def load_gt(infos, class_names=CLASSES):
    """-> ({token: [EvalBox dicts]}, {token: [rack boxes]}); attributes from gt_attr_names ('' without them)"""
    gt, racks = {}, {}
    for info in infos:
        boxes, rk = [], []
        names = list(info["gt_names"])
        for i, name in enumerate(names):
            x, y, z, l, w, h, yaw = np.asarray(info["gt_boxes"], np.float64)[i][:7]
            v = np.asarray(info["gt_velocity"], np.float64)[i]
            box = _box([x, y, z], [w, l, h], yaw, v)
            _to_global(box, info)
            if name == "static_object.bicycle_rack":
                rk.append(box)
            if name not in class_names:
                continue
            attr = str(info["gt_attr_names"][i]) if "gt_attr_names" in info else ""
            boxes.append(dict(sample_token=info["token"], translation=box["center"], size=box["wlh"], rotation=box["q"],
                              velocity=box["velocity"][:2], detection_name=name, attribute_name=attr,
                              num_pts=int(info["num_lidar_pts"][i]) + int(info["num_radar_pts"][i])))
        gt[info["token"]] = boxes
        racks[info["token"]] = rk
    return gt, racks


def points_in_box(box, point):
    w, l, h = box["wlh"]
    xs, ys, zs = [1, 1, 1, 1, -1, -1, -1, -1], [1, -1, -1, 1, 1, -1, -1, 1], [1, 1, -1, -1, 1, 1, -1, -1]
    corners = []
    for k in range(8):
        c = q_rotate(box["q"], [l / 2 * xs[k], w / 2 * ys[k], h / 2 * zs[k]])
        corners.append(np.array([c[0] + box["center"][0], c[1] + box["center"][1], c[2] + box["center"][2]]))
    p1, px, py, pz = corners[0], corners[4], corners[1], corners[3]
    i, j, k = px - p1, py - p1, pz - p1
    v = np.asarray(point) - p1
    iv, jv, kv = np.dot(i, v), np.dot(j, v), np.dot(k, v)
    return (0 <= iv <= np.dot(i, i)) and (0 <= jv <= np.dot(j, j)) and (0 <= kv <= np.dot(k, k))


def filter_boxes(boxes, racks, infos):
    ego = {info["token"]: info["ego2global_translation"] for info in infos}
    out = {}
    for token, bs in boxes.items():
        t = ego[token]
        kept = []
        for b in bs:
            ego_translation = [b["translation"][k] - t[k] for k in range(3)]
            ego_dist = np.sqrt(np.sum(np.array(ego_translation[:2]) ** 2))
            if not ego_dist < CLASS_RANGE[b["detection_name"]]:
                continue
            if b["num_pts"] == 0:
                continue
            if b["detection_name"] in ["bicycle", "motorcycle"]:
                if any(points_in_box(r, b["translation"]) for r in racks[token]):
                    continue
            kept.append(b)
        out[token] = kept
    return out


# ---------------------------------------------------------------- metrics
def center_distance(gt_box, pred_box):
    return np.linalg.norm(np.array(pred_box["translation"][:2]) - np.array(gt_box["translation"][:2]))


def velocity_l2(gt_box, pred_box):
    return np.linalg.norm(np.array(pred_box["velocity"]) - np.array(gt_box["velocity"]))


def angle_diff(x, y, period):
    diff = (x - y + period / 2) % period - period / 2
    if diff > np.pi:
        diff = diff - (2 * np.pi)
    return diff


def yaw_diff(gt_box, eval_box, period=2 * np.pi):
    return abs(angle_diff(quaternion_yaw(gt_box["rotation"]), quaternion_yaw(eval_box["rotation"]), period))


def attr_acc(gt_box, pred_box):
    if gt_box["attribute_name"] == "":
        return np.nan
    return float(gt_box["attribute_name"] == pred_box["attribute_name"])


def scale_iou(sample_annotation, sample_result):
    sa_size, sr_size = np.array(sample_annotation["size"]), np.array(sample_result["size"])
    min_wlh = np.minimum(sa_size, sr_size)
    intersection = np.prod(min_wlh)
    union = np.prod(sa_size) + np.prod(sr_size) - intersection
    return intersection / union


def cummean(x):
    if sum(np.isnan(x)) == len(x):
        return np.ones(len(x))
    sum_vals = np.nancumsum(x.astype(float))
    count_vals = np.cumsum(~np.isnan(x))
    return np.divide(sum_vals, count_vals, out=np.zeros_like(sum_vals), where=count_vals != 0)


def no_predictions():
    return dict(precision=np.zeros(101), confidence=np.zeros(101), **{k: np.ones(101) for k in TP_METRICS})


def accumulate(gt_boxes, pred_boxes, class_name, dist_th):
    all_gt = [b for bs in gt_boxes.values() for b in bs]
    npos = len([1 for b in all_gt if b["detection_name"] == class_name])
    if npos == 0:
        return no_predictions()
    pred_boxes_list = [b for bs in pred_boxes.values() for b in bs if b["detection_name"] == class_name]
    pred_confs = [b["detection_score"] for b in pred_boxes_list]
    sortind = [i for (v, i) in sorted((v, i) for (i, v) in enumerate(pred_confs))][::-1]
    tp, fp, conf = [], [], []
    match_data = {k: [] for k in TP_METRICS + ["conf"]}
    taken = set()
    for ind in sortind:
        pred_box = pred_boxes_list[ind]
        min_dist, match_gt_idx = np.inf, None
        for gt_idx, gt_box in enumerate(gt_boxes[pred_box["sample_token"]]):
            if gt_box["detection_name"] == class_name and (pred_box["sample_token"], gt_idx) not in taken:
                this_distance = center_distance(gt_box, pred_box)
                if this_distance < min_dist:
                    min_dist, match_gt_idx = this_distance, gt_idx
        if min_dist < dist_th:
            taken.add((pred_box["sample_token"], match_gt_idx))
            tp.append(1)
            fp.append(0)
            conf.append(pred_box["detection_score"])
            g = gt_boxes[pred_box["sample_token"]][match_gt_idx]
            match_data["trans_err"].append(center_distance(g, pred_box))
            match_data["vel_err"].append(velocity_l2(g, pred_box))
            match_data["scale_err"].append(1 - scale_iou(g, pred_box))
            match_data["orient_err"].append(yaw_diff(g, pred_box, period=np.pi if class_name == "barrier" else 2 * np.pi))
            match_data["attr_err"].append(1 - attr_acc(g, pred_box))
            match_data["conf"].append(pred_box["detection_score"])
        else:
            tp.append(0)
            fp.append(1)
            conf.append(pred_box["detection_score"])
    if len(match_data["trans_err"]) == 0:
        return no_predictions()
    tp, fp = np.cumsum(tp).astype(float), np.cumsum(fp).astype(float)
    conf = np.array(conf)
    prec = tp / (fp + tp)
    rec = tp / float(npos)
    rec_interp = np.linspace(0, 1, 101)
    prec = np.interp(rec_interp, rec, prec, right=0)
    conf = np.interp(rec_interp, rec, conf, right=0)
    md = dict(precision=prec, confidence=conf)
    for key in TP_METRICS:
        tmp = cummean(np.array(match_data[key]))
        md[key] = np.interp(conf[::-1], match_data["conf"][::-1], tmp[::-1])[::-1]
    return md


def max_recall_ind(md):
    non_zero = np.nonzero(md["confidence"])[0]
    return 0 if len(non_zero) == 0 else non_zero[-1]


def calc_ap(md):
    prec = np.copy(md["precision"])[round(100 * MIN_RECALL) + 1:]
    prec -= MIN_PRECISION
    prec[prec < 0] = 0
    return float(np.mean(prec)) / (1.0 - MIN_PRECISION)


def calc_tp(md, metric_name):
    first_ind, last_ind = round(100 * MIN_RECALL) + 1, max_recall_ind(md)
    if last_ind < first_ind:
        return 1.0
    return float(np.mean(md[metric_name][first_ind:last_ind + 1]))


def evaluate(results, infos, class_names=CLASSES):
    """-> dict(label_aps {cls: {th: ap}}, label_tp_errors {cls: {metric: v}}, mean_ap, tp_errors, nd_score)"""
    gt, racks = load_gt(infos, class_names)
    pred = filter_boxes(format_results(results, infos, class_names), racks, infos)
    gt = filter_boxes(gt, racks, infos)
    label_aps, label_tp = {}, {}
    for c in class_names:
        mds = {th: accumulate(gt, pred, c, th) for th in DIST_THS}
        label_aps[c] = {th: calc_ap(mds[th]) for th in DIST_THS}
        label_tp[c] = {}
        for m in TP_METRICS:
            if c in ["traffic_cone"] and m in ["attr_err", "vel_err", "orient_err"]:
                v = np.nan
            elif c in ["barrier"] and m in ["attr_err", "vel_err"]:
                v = np.nan
            else:
                v = calc_tp(mds[DIST_TH_TP], m)
            label_tp[c][m] = v
    mean_ap = float(np.mean([np.mean(list(d.values())) for d in label_aps.values()]))
    tp_errors = {m: float(np.nanmean([label_tp[c][m] for c in class_names])) for m in TP_METRICS}
    tp_scores = {m: max(0.0, 1.0 - tp_errors[m]) for m in TP_METRICS}
    nds = float(MEAN_AP_WEIGHT * mean_ap + np.sum(list(tp_scores.values()))) / float(MEAN_AP_WEIGHT + len(tp_scores))
    return dict(label_aps=label_aps, label_tp_errors=label_tp, mean_ap=mean_ap, tp_errors=tp_errors, nd_score=nds)
