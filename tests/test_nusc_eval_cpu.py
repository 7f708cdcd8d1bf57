"""nuScenes detection evaluation, float64 host path (uni3detr_amd/nuscenes_eval.py): against the loop-by-loop restatement in nusc_ref.py,
hand-derived cases, the conversion, the filters, the errors and the output format."""
import json
import math
import warnings

import numpy as np
import pytest

import nusc_ref
from uni3detr_amd import nuscenes_eval as ne
from uni3detr_amd.synth import nusc_samples

P = "pts_bbox_NuScenes"


def _ref(results, infos, class_names=ne.CLASSES):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return nusc_ref.evaluate(results, infos, class_names)


def _host(results, infos, class_names=ne.CLASSES):
    tab = ne._Tables(class_names)
    enc = ne._Encoded(tab)
    for r, i in zip(results, infos):
        enc.add_gt(i)
        enc.add_pred(r)
    return ne.evaluate_encoded(enc.arrays(), tab, "cpu"), tab, enc


def _info(token="s0", e2g_q=(1.0, 0.0, 0.0, 0.0), e2g_t=(1000.0, 1500.0, 0.0), l2e_q=(1.0, 0.0, 0.0, 0.0), l2e_t=(0.0, 0.0, 0.0), gt=(),
          attrs=True):
    """gt: tuples (name, x, y, z (gravity), l, w, h, yaw, vx, vy, num_lidar_pts[, attribute])"""
    info = dict(token=token, lidar2ego_rotation=list(l2e_q), lidar2ego_translation=list(l2e_t), ego2global_rotation=list(e2g_q),
                ego2global_translation=list(e2g_t), gt_names=np.array([g[0] for g in gt]),
                gt_boxes=np.array([g[1:8] for g in gt], np.float64).reshape(-1, 7), gt_velocity=np.array([g[8:10] for g in gt], np.float64).reshape(-1, 2),
                num_lidar_pts=np.array([g[10] for g in gt], np.int64), num_radar_pts=np.zeros(len(gt), np.int64))
    if attrs:
        info["gt_attr_names"] = np.array([g[11] if len(g) > 11 else "" for g in gt])
    return info


def _res(boxes, scores, labels):
    return dict(boxes_3d=np.asarray(boxes, np.float64).reshape(-1, 9), scores_3d=np.asarray(scores, np.float64),
                labels_3d=np.asarray(labels, np.int64))


def _gt_as_pred(info, class_names=ne.CLASSES):
    keep = [i for i, n in enumerate(info["gt_names"]) if n in class_names and info["num_lidar_pts"][i] + info["num_radar_pts"][i] > 0]
    b = np.asarray(info["gt_boxes"], np.float64)[keep]
    v = np.nan_to_num(np.asarray(info["gt_velocity"], np.float64)[keep])
    boxes = np.concatenate([b[:, :2], b[:, 2:3] - b[:, 5:6] / 2, b[:, 3:7], v], 1)
    return _res(boxes, np.ones(len(keep)), [list(class_names).index(info["gt_names"][i]) for i in keep])


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_host_path_equals_loop_reference(seed):
    infos, results = nusc_samples(12, preds_per_sample=50, seed=seed)
    ref = _ref(results, infos)
    h, tab, _ = _host(results, infos)
    la, lt, mean_ap, te, nds = ne.summarize(h["ap"], h["tp_err"], tab.names)
    n_checked = 0
    for c in tab.names:
        for th in ne.DIST_THS:
            assert abs(la[c][th] - ref["label_aps"][c][th]) <= 1e-12, (c, th)
        for m in ne.TP_METRICS:
            a, b = lt[c][m], ref["label_tp_errors"][c][m]
            assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-12, (c, m, a, b)
            n_checked += not math.isnan(a)
    for m in ne.TP_METRICS:
        assert abs(te[m] - ref["tp_errors"][m]) <= 1e-12, m
    assert abs(mean_ap - ref["mean_ap"]) <= 1e-12 and abs(nds - ref["nd_score"]) <= 1e-12
    assert 0.1 < mean_ap < 0.9 and n_checked >= 40 and h["tp"].sum() > 100


def test_gt_fed_back_as_predictions_is_perfect():
    infos, _ = nusc_samples(8, seed=21)
    results = [_gt_as_pred(i) for i in infos]
    r = ne.nuscenes_eval(results, infos, device="cpu", logger="silent")
    for c in ne.CLASSES:
        for th in ne.DIST_THS:
            assert r[f"{P}/{c}_AP_dist_{th}"] == 1.0, (c, th)
        for m in ne.TP_METRICS:
            v = r[f"{P}/{c}_{m}"]
            assert math.isnan(v) if (c == "traffic_cone" and m != "trans_err" and m != "scale_err") or (c == "barrier" and m in ("vel_err", "attr_err")) else v == 0.0, (c, m, v)
    assert abs(r[f"{P}/NDS"] - 1.0) <= 1e-12 and abs(r[f"{P}/mAP"] - 1.0) <= 1e-12


def test_pure_shift_of_1_5_m():
    info = _info(gt=[("car", 10.0, 5.0, -1.0, 4.0, 2.0, 1.5, 0.3, 0.0, 0.0, 10, "vehicle.parked")])
    res = _res([[11.5, 5.0, -1.75, 4.0, 2.0, 1.5, 0.3, 0.0, 0.0]], [0.8], [0])
    r = ne.nuscenes_eval([res], [info], class_names=["car"], device="cpu", logger="silent")
    assert r[f"{P}/car_AP_dist_0.5"] == 0.0 and r[f"{P}/car_AP_dist_1.0"] == 0.0
    assert r[f"{P}/car_AP_dist_2.0"] == 1.0 and r[f"{P}/car_AP_dist_4.0"] == 1.0
    assert r[f"{P}/car_trans_err"] == 1.5 and r[f"{P}/car_scale_err"] == 0.0 and r[f"{P}/car_orient_err"] == 0.0
    h, _, _ = _host([res], [info], ["car"])
    assert abs(h["tp_err"][0, 0] - 1.5) <= 1e-12 and abs(r[f"{P}/mAP"] - 0.5) <= 1e-12


def test_yaw_flipped_by_pi_is_free_for_barrier_only():
    gt = [("car", 10.0, 5.0, -1.0, 4.0, 2.0, 1.5, 0.3, 0.0, 0.0, 10, "vehicle.parked"),
          ("barrier", -8.0, 3.0, -1.0, 2.5, 0.5, 1.0, -0.7, 0.0, 0.0, 10, "")]
    res = _res([[10.0, 5.0, -1.75, 4.0, 2.0, 1.5, 0.3 + np.pi, 0.0, 0.0], [-8.0, 3.0, -1.5, 2.5, 0.5, 1.0, -0.7 + np.pi, 0.0, 0.0]],
               [0.9, 0.7], [0, 1])
    h, _, _ = _host([res], [_info(gt=gt)], ["car", "barrier"])
    assert abs(h["tp_err"][0, 2] - np.pi) <= 1e-12 and h["tp_err"][1, 2] <= 1e-12


def test_traffic_cone_and_barrier_nans():
    infos, results = nusc_samples(4, seed=22)
    r = ne.nuscenes_eval(results, infos, device="cpu", logger="silent")
    for m in ("orient_err", "vel_err", "attr_err"):
        assert math.isnan(r[f"{P}/traffic_cone_{m}"])
    for m in ("vel_err", "attr_err"):
        assert math.isnan(r[f"{P}/barrier_{m}"])
    for m in ("trans_err", "scale_err"):
        assert not math.isnan(r[f"{P}/traffic_cone_{m}"])
    assert not math.isnan(r[f"{P}/barrier_orient_err"]) and not math.isnan(r[f"{P}/mAOE"])


def test_equal_score_tie_puts_the_later_sample_first():
    # sample 0: a false positive, sample 1: a true positive, both at score 0.5.  The later (sample, position) ranks first:
    # rec = [0.5, 0.5], prec = [1, 0.5] -> interpolated precision 1 below recall 0.5, 0.5 at 0.5, then 0.
    gt = [("car", 10.0, 0.0, -1.0, 4.0, 2.0, 1.5, 0.0, 0.0, 0.0, 10, "vehicle.parked")]
    infos = [_info("a", gt=gt), _info("b", gt=gt)]
    res = [_res([[30.0, 0.0, -1.75, 4.0, 2.0, 1.5, 0.0, 0.0, 0.0]], [0.5], [0]), _res([[10.0, 0.0, -1.75, 4.0, 2.0, 1.5, 0.0, 0.0, 0.0]], [0.5], [0])]
    h, _, _ = _host(res, infos, ["car"])
    want = (39 * 0.9 + 0.4) / 90 / 0.9
    assert np.all(np.abs(h["ap"][0] - want) <= 1e-12), h["ap"][0]
    # the other order (the TP in the earlier sample) changes AP: the FP ranks first
    h2, _, _ = _host(res[::-1], infos[::-1], ["car"])
    other = sum(max(q / 100 - 0.1, 0.0) for q in range(11, 51)) / 90 / 0.9
    assert np.all(np.abs(h2["ap"][0] - other) <= 1e-12) and abs(want - other) > 0.1
    assert abs(_ref(res, infos, ["car"])["label_aps"]["car"][2.0] - want) <= 1e-12


def test_class_range_filters_ego_radius_and_ego_dist():
    # ego2global pitched by 0.1 rad about y: the ego-frame xy radius and the global ego_dist differ
    th = 0.1
    pitch = (math.cos(th / 2), 0.0, math.sin(th / 2), 0.0)
    gt = [("car", 49.99, 0.0, 0.0, 4.0, 2.0, 1.5, 0.0, 0.0, 0.0, 10),        # kept (radius 49.99, ego_dist 49.74)
          ("car", 50.2, 0.0, 0.0, 4.0, 2.0, 1.5, 0.0, 0.0, 0.0, 10),         # GT: ego_dist 49.95 < 50, kept
          ("car", 49.9, 0.0, 10.0, 4.0, 2.0, 1.5, 0.0, 0.0, 0.0, 10)]        # ego_dist 50.65: dropped
    info = _info(e2g_q=pitch, gt=gt)
    boxes = [[g[1], g[2], g[3] - 0.75, 4.0, 2.0, 1.5, 0.0, 0.0, 0.0] for g in gt]
    res = _res(boxes, [0.9, 0.8, 0.7], [0, 0, 0])
    tab = ne._Tables(["car"])
    enc = ne._Encoded(tab)
    enc.add_gt(info)
    enc.add_pred(res)
    pred, pc, gtr, gc = ne.host_global(enc.arrays(), tab)
    assert gc == [2] and np.allclose(gtr[:, 0] - 1000.0, [49.99 * math.cos(th), 50.2 * math.cos(th)])
    assert pc == [1] and abs(pred[0, 0] - 1000.0 - 49.99 * math.cos(th)) < 1e-9       # radius 50.2 > 50 and ego_dist 50.65 dropped
    subm = ne.lidar_results_to_nusc([res], [info], ["car"])["results"]["s0"]
    assert len(subm) == 2                                                              # the submission applies the radius drop only


def test_gt_without_points_is_dropped():
    gt = [("car", 10.0, 0.0, -1.0, 4.0, 2.0, 1.5, 0.0, 0.0, 0.0, 0), ("car", 20.0, 0.0, -1.0, 4.0, 2.0, 1.5, 0.0, 0.0, 0.0, 3)]
    tab = ne._Tables(["car"])
    enc = ne._Encoded(tab)
    enc.add_gt(_info(gt=gt))
    enc.add_pred(_res(np.zeros((0, 9)), [], []))
    _, _, gtr, gc = ne.host_global(enc.arrays(), tab)
    assert gc == [1] and abs(gtr[0, 0] - 1020.0) < 1e-9


def test_bicycle_inside_a_rack_is_dropped():
    rack = ("static_object.bicycle_rack", 10.0, 10.0, -1.0, 4.0, 1.5, 1.2, 0.5, 0.0, 0.0, 5)
    gt = [rack, ("bicycle", 10.5, 10.2, -1.1, 1.7, 0.6, 1.0, 0.3, 0.0, 0.0, 5, "cycle.without_rider"),     # inside: dropped
          ("car", 10.0, 10.0, -1.0, 4.0, 2.0, 1.5, 0.0, 0.0, 0.0, 5, "vehicle.parked"),                  # not a bike: kept
          ("motorcycle", 14.0, 10.0, -1.0, 2.1, 0.8, 1.5, 0.0, 0.0, 0.0, 5, "cycle.without_rider")]      # outside: kept
    info = _info(gt=gt)
    names = ["car", "bicycle", "motorcycle"]
    boxes = [[g[1], g[2], g[3] - g[6] / 2, g[4], g[5], g[6], g[7], 0.0, 0.0] for g in gt[1:]]
    res = _res(boxes, [0.9, 0.8, 0.7], [1, 0, 2])
    tab = ne._Tables(names)
    enc = ne._Encoded(tab)
    enc.add_gt(info)
    enc.add_pred(res)
    pred, pc, gtr, gc = ne.host_global(enc.arrays(), tab)
    assert gc == [2] and sorted(gtr[:, 10].tolist()) == [0.0, 2.0]
    assert pc == [2] and sorted(pred[:, 10].tolist()) == [0.0, 2.0]
    ref = _ref([res], [info], names)
    assert ref["label_aps"]["bicycle"][4.0] == 0.0 and ref["label_aps"]["car"][4.0] > 0.99


def test_attribute_heuristic_is_strict_at_0_2():
    info = _info(gt=[])
    boxes = [[5.0, 0.0, -1.0, 4.0, 2.0, 1.5, 0.0, 0.2, 0.0], [6.0, 0.0, -1.0, 4.0, 2.0, 1.5, 0.0, 0.0, 0.2000001],
             [7.0, 0.0, -1.0, 0.7, 0.7, 1.8, 0.0, 0.2, 0.0], [8.0, 0.0, -1.0, 11.0, 2.9, 3.5, 0.0, 0.0, 0.0],
             [9.0, 0.0, -1.0, 1.7, 0.6, 1.3, 0.0, 3.0, 0.0], [3.0, 0.0, -1.0, 0.4, 0.4, 1.1, 0.0, 3.0, 0.0]]
    names = ["car", "pedestrian", "bus", "bicycle", "traffic_cone"]
    res = _res(boxes, [0.5] * 6, [0, 0, 1, 2, 3, 4])
    got = [b["attribute_name"] for b in ne.lidar_results_to_nusc([res], [info], names)["results"]["s0"]]
    assert got == ["vehicle.parked", "vehicle.moving", "pedestrian.standing", "vehicle.stopped", "cycle.with_rider", ""]


def test_global_round_trip_against_closed_form_rotation():
    phi, T = 0.7, np.array([1234.5, 876.25, 3.0])
    info = _info(e2g_q=(math.cos(phi / 2), 0.0, 0.0, math.sin(phi / 2)), e2g_t=T, l2e_t=(1.0, -0.5, 1.8))
    box = [12.0, -3.0, -1.0, 4.0, 2.0, 1.6, 2.9, 1.5, -0.5]
    sub = ne.lidar_results_to_nusc([_res([box], [0.6], [0])], [info], ["car"])["results"]["s0"][0]
    c, s = math.cos(phi), math.sin(phi)
    e = np.array([box[0] + 1.0, box[1] - 0.5, box[2] + 0.8 + 1.8])
    want = np.array([c * e[0] - s * e[1], s * e[0] + c * e[1], e[2]]) + T
    assert np.abs(np.asarray(sub["translation"]) - want).max() <= 1e-9
    assert np.allclose(sub["size"], [2.0, 4.0, 1.6]) and np.allclose(sub["velocity"], [c * 1.5 + s * 0.5, s * 1.5 - c * 0.5])
    q = sub["rotation"]
    yaw = math.atan2(2 * (q[0] * q[3] + q[1] * q[2]), 1 - 2 * (q[2] ** 2 + q[3] ** 2))
    assert abs((yaw - (2.9 + phi) + math.pi) % (2 * math.pi) - math.pi) <= 1e-12
    rec, _ = ne.to_global(np.array([box]), np.array([0]), np.array([0.6]), None, [1], ne._calib(info)[None], True, ne._Tables(["car"]))
    assert np.abs(rec[0, :3] - want).max() <= 1e-9 and abs((rec[0, 6] - yaw + math.pi) % (2 * math.pi) - math.pi) <= 1e-12


def test_errors():
    info = _info(gt=[("car", 10.0, 0.0, -1.0, 4.0, 2.0, 1.5, 0.0, 0.0, 0.0, 10)])
    many = _res(np.tile([[5.0, 0.0, -1.0, 4.0, 2.0, 1.5, 0.0, 0.0, 0.0]], (501, 1)), np.full(501, 0.5), np.zeros(501))
    with pytest.raises(ValueError):
        ne.nuscenes_eval([many], [info], device="cpu")
    ne.nuscenes_eval([dict(many, boxes_3d=many["boxes_3d"][:500], scores_3d=many["scores_3d"][:500], labels_3d=many["labels_3d"][:500])],
                     [info], device="cpu", logger="silent")
    with pytest.raises(ValueError):
        ne.nuscenes_eval([_res([[5.0, 0.0, -1.0, 4.0, 2.0, 1.5, 0.0, 0.0, 0.0]], [np.nan], [0])], [info], device="cpu")
    with pytest.raises(ValueError):
        ne.nuscenes_eval([_res([[5.0, 0.0, -1.0, 4.0, 2.0, 1.5, 0.0, 0.0, 0.0]], [0.5], [10])], [info], device="cpu")
    with pytest.raises(ValueError):
        ne.nuscenes_eval([_res([[5.0, 0.0, -1.0, 4.0, 2.0, 1.5, 0.0, 0.0, 0.0]], [0.5], [1])], [info], class_names=["car"], device="cpu")
    with pytest.raises(ValueError):
        ne.NuScenesEvaluator(["car", "van"], device="cpu")
    with pytest.raises(NotImplementedError):
        ne.nuscenes_eval([_res(np.zeros((0, 9)), [], [])], [info], eval_version="detection_cvpr_2021", device="cpu")


def test_ret_dict_keys_and_rounding():
    infos, results = nusc_samples(5, seed=23)
    r = ne.nuscenes_eval([dict(pts_bbox=x) for x in results], infos, device="cpu", logger="silent")
    want = set()
    for c in ne.CLASSES:
        want |= {f"{P}/{c}_AP_dist_{th}" for th in ("0.5", "1.0", "2.0", "4.0")}
        want |= {f"{P}/{c}_{m}" for m in ne.TP_METRICS}
    want |= {f"{P}/{m}" for m in ("mATE", "mASE", "mAOE", "mAVE", "mAAE", "NDS", "mAP")}
    assert set(r) == want
    for k, v in r.items():
        if k.endswith(("/NDS", "/mAP")) or math.isnan(v):
            continue
        assert v == float("{:.4f}".format(v)), k
    h, tab, _ = _host(results, infos)
    _, _, mean_ap, _, nds = ne.summarize(h["ap"], h["tp_err"], tab.names)
    assert r[f"{P}/mAP"] == mean_ap and r[f"{P}/NDS"] == nds and r[f"{P}/mAP"] != float("{:.4f}".format(mean_ap))
    r2 = ne.nuscenes_eval(results, infos, result_name="img_bbox", device="cpu", logger="silent")
    assert set(r2) == {k.replace("pts_bbox", "img_bbox") for k in want}


def test_without_gt_attributes_attr_err_is_nan(caplog):
    infos, results = nusc_samples(4, seed=24)
    bare = [{k: v for k, v in i.items() if k != "gt_attr_names"} for i in infos]
    with caplog.at_level("WARNING"):
        r = ne.nuscenes_eval(results, bare, device="cpu", logger="silent")
    assert "gt_attr_names" in caplog.text
    assert all(math.isnan(r[f"{P}/{c}_attr_err"]) for c in ne.CLASSES) and math.isnan(r[f"{P}/mAAE"])
    full = ne.nuscenes_eval(results, infos, device="cpu", logger="silent")
    assert abs(r[f"{P}/NDS"] - (full[f"{P}/NDS"] - max(0.0, 1.0 - full[f"{P}/mAAE"]) / 10)) <= 1e-4
    # the literal devkit reads '' attributes as attr_err 1 (cummean of all-NaN is ones): that term scores 0 as well
    assert abs(r[f"{P}/NDS"] - _ref(results, bare)["nd_score"]) <= 1e-12


def test_submission_format(tmp_path):
    infos, results = nusc_samples(6, seed=25)
    sub = ne.lidar_results_to_nusc(results, infos)
    assert list(sub["results"]) == [i["token"] for i in infos] and sub["meta"]["use_lidar"]
    n = 0
    for res, info in zip(results, infos):
        b = res["boxes_3d"].astype(np.float64)
        for box in sub["results"][info["token"]]:
            assert box["sample_token"] == info["token"] and abs(np.linalg.norm(box["rotation"]) - 1.0) <= 1e-12
            k = int(np.argmin(np.abs(res["scores_3d"].astype(np.float64) - box["detection_score"]) + np.abs(b[:, 5] - box["size"][2])))
            assert np.allclose(box["size"], b[k, [4, 3, 5]])                       # wlh
            assert box["detection_name"] in ne.CLASSES and len(box["velocity"]) == 2
            n += 1
    assert n > 100
    path = ne.format_results(results, infos, str(tmp_path / "out"))
    with open(path) as f:
        assert json.load(f) == json.loads(json.dumps(sub))
