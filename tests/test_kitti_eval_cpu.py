"""KITTI detection evaluation, host path (uni3detr_amd/kitti_eval.py, device="cpu"): hand-derivable pins of the contract, closed-form
overlaps, the LiDAR -> KITTI conversion round trip, GT fed back as predictions, and input errors."""
import numpy as np
import pytest

from uni3detr_amd import kitti_eval as ke
from uni3detr_amd.synth import kitti_scenes

CLASSES = ["Pedestrian", "Cyclist", "Car"]


def _anno(objs, score=None):
    """objs: (name, bbox, loc, dims (l, h, w), ry[, occluded, truncated]) -> KITTI anno dict (alpha = ry - atan2(x, z))."""
    n = len(objs)
    a = dict(name=np.array([o[0] for o in objs]), bbox=np.array([o[1] for o in objs], np.float64).reshape(n, 4),
             location=np.array([o[2] for o in objs], np.float64).reshape(n, 3),
             dimensions=np.array([o[3] for o in objs], np.float64).reshape(n, 3), rotation_y=np.array([o[4] for o in objs], np.float64),
             occluded=np.array([o[5] if len(o) > 5 else 0 for o in objs]), truncated=np.array([o[6] if len(o) > 6 else 0.0 for o in objs]))
    a["alpha"] = a["rotation_y"] - np.arctan2(a["location"][:, 0], a["location"][:, 2]) if n else np.zeros(0)
    if score is not None:
        a["score"] = np.asarray(score, np.float64)
    return a


def _car(x=0.0, z=20.0, top=100.0, height=100.0, name="Car", **kw):
    return (name, [500.0 + 10 * x, top, 600.0 + 10 * x, top + height], [x, 1.6, z], [3.9, 1.5, 1.6], 0.3) + tuple(kw.values())


def _eval(gt, dt, classes=("Car",), types=("bbox", "bev", "3d")):
    return ke.kitti_eval(gt, dt, list(classes), list(types), device="cpu")[1]


def _records(gt_annos, dt_annos, classes=("Car",), metrics=(0, 1, 2), aos=False):
    gt, gc = ke._encode_all(gt_annos, True)
    dt, dc = ke._encode_all(dt_annos, False)
    return ke.host_core(dt, dc, gt, gc, ke._class_ids(classes), list(metrics), aos)


def _group(classes, metrics, ci, d, m, o):
    return ((ci * 3 + d) * len(metrics) + list(metrics).index(m)) * 2 + o


# ---------------------------------------------------------------------------------------------------------------
# hand-derivable pins
# ---------------------------------------------------------------------------------------------------------------
def test_one_gt_one_perfect_detection():
    g = _car()
    r = _eval([_anno([g])], [_anno([g], [0.9])])
    for m in ("2D", "BEV", "3D"):
        for d in ("easy", "moderate", "hard"):
            assert r[f"KITTI/Car_{m}_AP11_{d}_strict"] == pytest.approx(100 / 11, abs=1e-12)
            assert r[f"KITTI/Car_{m}_AP40_{d}_strict"] == 0.0
    assert not any("Overall" in k for k in r)                 # one class: no Overall keys


def test_forty_gt_distinct_scores_give_forty_thresholds():
    gts, dts = [], []
    for k in range(40):
        g = _car()
        gts.append(_anno([g]))
        dts.append(_anno([g], [0.1 + 0.02 * k]))
    res = _records(gts, dts)
    assert set(res["nthr"].tolist()) == {40}
    r = _eval(gts, dts)
    assert r["KITTI/Car_3D_AP40_moderate_strict"] == pytest.approx(97.5, abs=1e-9)
    assert r["KITTI/Car_3D_AP11_moderate_strict"] == pytest.approx(1000 / 11, abs=1e-9)


def test_van_detected_as_car_is_neither_tp_nor_fp():
    van, car = _car(x=-20, name="Van"), _car(x=20)
    gt = [_anno([van, car])]
    dt = [_anno([("Car",) + van[1:], car], [0.95, 0.9])]
    res = _records(gt, dt)
    g = _group(["Car"], (0, 1, 2), 0, 1, 2, 0)
    assert res["nthr"][g] == 1 and res["thr"][g, 0] == 0.9
    assert res["tot"][g, :, 0].tolist() == [1, 0, 0]          # tp, fp, fn
    assert _eval(gt, dt)["KITTI/Car_3D_AP11_moderate_strict"] == pytest.approx(100 / 11)


def test_detection_below_the_height_limit_is_ignored():
    car = _car()
    small = ("Car", [100.0, 150.0, 130.0, 170.0], [-20.0, 1.6, 40.0], [3.9, 1.5, 1.6], 0.0)      # 20 px high, away from the car
    gt = [_anno([car])]
    dt = [_anno([car, small], [0.9, 0.95])]
    res = _records(gt, dt)
    for m in (0, 1, 2):
        g = _group(["Car"], (0, 1, 2), 0, 1, m, 0)
        assert res["tot"][g, :, 0].tolist() == [1, 0, 0]
    big = ("Car",) + ((100.0, 150.0, 130.0, 200.0),) + small[2:]                                 # 50 px: now an FP
    res = _records(gt, [_anno([car, big], [0.9, 0.95])])
    assert res["tot"][_group(["Car"], (0, 1, 2), 0, 1, 2, 0), :, 0].tolist() == [1, 1, 0]


def test_detection_inside_dontcare_is_fp_for_bev_only():
    car = _car()
    dc = ("DontCare", [100.0, 120.0, 200.0, 200.0], [-1000.0, -1000.0, -1000.0], [-1.0, -1.0, -1.0], -10.0)
    inside = ("Car", [110.0, 125.0, 190.0, 195.0], [-15.0, 1.6, 15.0], [3.9, 1.5, 1.6], 0.0)
    gt = [_anno([car, dc])]
    dt = [_anno([car, inside], [0.9, 0.95])]
    res = _records(gt, dt)
    assert res["dc_iof"][0][1] == pytest.approx(1.0) and res["dc_iof"][0][0] == 0.0
    bbox, bev = _group(["Car"], (0, 1, 2), 0, 1, 0, 0), _group(["Car"], (0, 1, 2), 0, 1, 1, 0)
    assert res["tot"][bbox, :, 0].tolist() == [1, 0, 0]
    assert res["tot"][bev, :, 0].tolist() == [1, 1, 0]
    r = _eval(gt, dt)
    assert r["KITTI/Car_2D_AP11_moderate_strict"] == pytest.approx(100 / 11)
    assert r["KITTI/Car_BEV_AP11_moderate_strict"] == pytest.approx(50 / 11)


def test_pass1_ties_go_to_the_lower_index():
    ov = np.array([[0.8], [0.9], [0.95]])
    assert ke.pass1(ov, np.array([0]), np.array([0, 0, 0]), np.array([0.5, 0.7, 0.7]), 0.7) == [0.7]
    # the same through the whole path: two equal-score detections of one GT, the lower index is the TP, the other an FP
    car = _car()
    near = ("Car", [502.0, 101.0, 602.0, 201.0], [0.05, 1.6, 20.05], [3.9, 1.5, 1.6], 0.3)
    res = _records([_anno([car])], [_anno([near, car], [0.8, 0.8])])
    g = _group(["Car"], (0, 1, 2), 0, 1, 0, 0)
    assert res["thr"][g, 0] == np.float64(0.8) and res["tot"][g, :, 0].tolist() == [1, 1, 0]


def test_class_without_valid_gt_has_ap_zero():
    car = _car()
    cyc = ("Cyclist", [200.0, 100.0, 240.0, 190.0], [-8.0, 1.6, 15.0], [1.75, 1.7, 0.6], 0.0)
    r = _eval([_anno([car])], [_anno([car, cyc], [0.9, 0.8])], classes=("Car", "Cyclist"))
    assert all(v == 0.0 for k, v in r.items() if "Cyclist" in k)
    assert r["KITTI/Overall_3D_AP11_moderate"] == pytest.approx((100 / 11) / 2)


def test_aos_is_on_only_with_valid_alpha():
    car = _car()
    r = _eval([_anno([car])], [_anno([car], [0.9])])
    assert r["KITTI/Car_AOS_AP11_moderate_strict"] == pytest.approx(100 / 11)
    dt = _anno([car], [0.9])
    dt["alpha"] = np.array([-10.0])
    assert not any("AOS" in k for k in _eval([_anno([car])], [dt]))
    # scenes without GT are skipped when looking for a valid first GT alpha
    r = _eval([_anno([]), _anno([car])], [_anno([], []), _anno([car], [0.9])])
    assert "KITTI/Car_AOS_AP40_hard_loose" in r


# ---------------------------------------------------------------------------------------------------------------
# overlaps against closed forms
# ---------------------------------------------------------------------------------------------------------------
def test_image_iou_closed_form():
    a = np.array([[0.0, 0.0, 10.0, 10.0]])
    b = np.array([[5.0, 0.0, 15.0, 10.0], [10.0, 0.0, 20.0, 10.0], [2.0, 2.0, 4.0, 4.0]])
    assert ke.image_box_iou(a, b)[0].tolist() == pytest.approx([1 / 3, 0.0, 0.04])
    assert ke.image_box_iou(b[2:], a, criterion=0)[0, 0] == 1.0


def test_bev_and_3d_iou_closed_form():
    def box(x, y, z, l, h, w, ry):
        return np.array([[x, y, z, l, h, w, ry]], np.float64)
    a = box(0, 0, 0, 4, 1, 2, 0)
    bev, d3 = ke.box_overlaps(a, box(2, 0, 0, 4, 1, 2, 0))                    # shifted by l/2 along x: 4 / (8 + 8 - 4)
    assert bev[0, 0] == pytest.approx(1 / 3) and d3[0, 0] == pytest.approx(1 / 3)
    bev, _ = ke.box_overlaps(a, box(0, 0, 0, 4, 1, 2, np.pi / 2))             # turned by 90 degrees: a 2 x 2 square in common
    assert bev[0, 0] == pytest.approx(4 / 12)
    bev, _ = ke.box_overlaps(a, box(1, 0, 0.5, 4, 1, 2, np.pi / 2))
    assert bev[0, 0] == pytest.approx(4 / 12)                                # (|dx| <= 1, |dz| <= 1 keeps the square inside both)
    _, d3 = ke.box_overlaps(a, box(0, -2, 0, 4, 1, 2, 0))                    # heights [-1, 0] and [-3, -2]: disjoint
    assert d3[0, 0] == 0.0
    _, d3 = ke.box_overlaps(a, box(0, -0.5, 0, 4, 1, 2, 0))                  # half the height in common: 4 / (8 + 8 - 4)
    assert d3[0, 0] == pytest.approx(1 / 3)
    bev, d3 = ke.box_overlaps(a, box(0, 0, 0, -1, -1, -1, -10))              # DontCare rows overlap nothing
    assert bev[0, 0] == 0.0 and d3[0, 0] == 0.0


# ---------------------------------------------------------------------------------------------------------------
# LiDAR -> KITTI conversion
# ---------------------------------------------------------------------------------------------------------------
def test_lidar_results_to_kitti_round_trip():
    infos, _ = kitti_scenes(12, seed=3)
    checked, dropped = 0, 0
    for info in infos:
        a = info["annos"]
        keep = a["name"] != "DontCare"
        loc, dims, ry = a["location"][keep], a["dimensions"][keep], a["rotation_y"][keep]
        T = info["calib"]["R0_rect"] @ info["calib"]["Tr_velo_to_cam"]
        p = np.concatenate([loc, np.ones((len(loc), 1))], 1) @ np.linalg.inv(T).T
        lid = np.concatenate([p[:, :3], dims[:, [0, 2, 1]], (-ry - np.pi / 2)[:, None]], 1)
        # two boxes that must drop: behind the camera (outside the image) and beyond pcd_limit_range's x
        lid = np.concatenate([lid, [[-20.0, 0.0, -1.0, 4.0, 1.6, 1.5, 0.0], [75.0, 0.0, -1.0, 4.0, 1.6, 1.5, 0.0]]])
        res = dict(boxes_3d=lid, scores_3d=np.linspace(0.1, 0.9, len(lid)).astype(np.float32),
                   labels_3d=np.full(len(lid), 2))
        out = ke.lidar_results_to_kitti([res], [info], CLASSES)[0]
        inside = ((lid[:, :3] > [0, -40, -3]) & (lid[:, :3] < [70.4, 40, 0])).all(1)
        assert len(out["name"]) == int(inside[:-2].sum())
        dropped += 2
        sel = np.nonzero(inside[:-2])[0]
        if sel.size == 0:
            continue
        assert np.abs(out["location"] - loc[sel]).max() < 1e-4
        assert np.abs(out["dimensions"] - dims[sel]).max() < 1e-4
        assert np.abs(np.cos(out["rotation_y"]) - np.cos(ry[sel])).max() < 1e-4
        assert np.abs(np.sin(out["rotation_y"]) - np.sin(ry[sel])).max() < 1e-4
        assert np.abs(out["bbox"] - a["bbox"][keep][sel]).max() < 1e-4
        assert np.all(out["name"] == "Car") and np.all(out["truncated"] == 0) and np.all(out["occluded"] == 0)
        checked += len(sel)
    assert checked > 40 and dropped == 24


# ---------------------------------------------------------------------------------------------------------------
# GT fed back as predictions
# ---------------------------------------------------------------------------------------------------------------
def test_gt_as_predictions():
    infos, _ = kitti_scenes(40, seed=5)
    rng = np.random.default_rng(0)
    gt_annos = [i["annos"] for i in infos]
    dt_annos = []
    for a in gt_annos:
        d = dict(a)
        d["score"] = rng.permutation(len(a["name"])).astype(np.float64) / 64 + rng.integers(0, 1000) / 1000
        dt_annos.append(d)
    res = _records(gt_annos, dt_annos, CLASSES)
    gfid, gmet, _ = ke._groups(ke._class_ids(CLASSES), [0, 1, 2])
    nonempty = 0
    for g in range(len(gfid)):
        nv, nt = int(res["nvalid"][gfid[g]]), int(res["nthr"][g])
        if nv == 0:
            assert nt == 0 and not res["ap"][g].any()
            continue
        nonempty += 1
        valid = res["gt_flag"][gfid[g]] == 0
        scores = np.concatenate([d["score"] for d in dt_annos])[valid]
        assert nt == len(ke.get_thresholds(scores, nv))
        thr = res["thr"][g, :nt]
        assert np.all(res["tot"][g, 1, :nt] == 0)
        assert np.array_equal(res["tot"][g, 0, :nt], (scores[None, :] >= thr[:, None]).sum(1))
        assert res["ap"][g, 0] == pytest.approx(len(range(0, nt, 4)) / 11 * 100)
        assert res["ap"][g, 1] == pytest.approx((nt - 1) / 40 * 100)
    assert nonempty >= 30


# ---------------------------------------------------------------------------------------------------------------
# errors and empty input
# ---------------------------------------------------------------------------------------------------------------
def test_errors_and_empty_scenes():
    car = _car()
    for bad in (["Van"], ["Truck"], [3], ["Car", "Person_sitting"]):
        with pytest.raises(ValueError):
            _eval([_anno([car])], [_anno([car], [0.9])], classes=bad)
    with pytest.raises(ValueError):
        _eval([_anno([car])], [_anno([car], [np.nan])])
    with pytest.raises(ValueError):
        _eval([_anno([car])], [_anno([car], [np.inf])])
    dc = ("DontCare", [100.0, 120.0, 200.0, 200.0], [-1000.0, -1000.0, -1000.0], [-1.0, -1.0, -1.0], -10.0)
    r = _eval([_anno([]), _anno([dc]), _anno([car])], [_anno([], []), _anno([], []), _anno([car], [0.9])], classes=(0, 1, 2))
    assert r["KITTI/Car_3D_AP11_easy_strict"] == pytest.approx(100 / 11)
    r = _eval([_anno([]), _anno([dc])], [_anno([], []), _anno([car], [0.5])], classes=CLASSES)
    assert all(v == 0.0 for v in r.values())
