"""nuScenes detection evaluation on the device (csrc/nusc_eval.hip through uni3detr_amd/nuscenes_eval.py) against the float64 host path."""
import math

import numpy as np
import pytest
import torch

from uni3detr_amd import nuscenes_eval as ne
from uni3detr_amd.eval_common import offsets
from uni3detr_amd.synth import nusc_samples

pytestmark = pytest.mark.gpu
P = "pts_bbox_NuScenes"


def _encoded(infos, results, class_names=ne.CLASSES):
    tab = ne._Tables(class_names)
    enc = ne._Encoded(tab)
    for r, i in zip(results, infos):
        enc.add_gt(i)
        enc.add_pred(r)
    return tab, enc.arrays()


def _same(got, want, tol=1e-12):
    assert set(got) == set(want), set(got) ^ set(want)
    for k in want:
        a, b = got[k], want[k]
        assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= tol, (k, a, b)


def _gt_as_pred(info):
    keep = [i for i, n in enumerate(info["gt_names"]) if n in ne.CLASSES and info["num_lidar_pts"][i] + info["num_radar_pts"][i] > 0]
    b = np.asarray(info["gt_boxes"], np.float64)[keep]
    v = np.nan_to_num(np.asarray(info["gt_velocity"], np.float64)[keep])
    boxes = np.concatenate([b[:, :2], b[:, 2:3] - b[:, 5:6] / 2, b[:, 3:7], v], 1)
    return dict(boxes_3d=boxes, scores_3d=np.ones(len(keep)), labels_3d=np.asarray([ne.CLASSES.index(info["gt_names"][i]) for i in keep]))


def test_device_global_boxes_match_host(cuda):
    infos, results = nusc_samples(40, seed=31)
    tab, a = _encoded(infos, results)
    hp, hpc, hg, hgc = ne.host_global(a, tab)
    u = ne._upload_encoded(a, cuda)
    dp, dpo, dg, dgo = ne.device_global(u["p_rows"], u["p_score"], u["p_lab"], u["p_off"], u["g_rows"], u["g_cls"], u["g_pts"], u["g_attr"],
                                        u["g_off"], u["calib"], ne._dev_tables(tab, cuda))
    assert np.diff(dpo.cpu().numpy()).tolist() == hpc and np.diff(dgo.cpu().numpy()).tolist() == hgc
    for d, h in ((dp, hp), (dg, hg)):
        d = d.cpu().numpy()
        assert np.abs(d[:, :6] - h[:, :6]).max() <= 1e-9
        dyaw = (d[:, 6] - h[:, 6] + np.pi) % (2 * np.pi) - np.pi
        assert np.abs(dyaw).max() <= 1e-12
        assert np.allclose(d[:, 7:9], h[:, 7:9], atol=1e-12, rtol=0, equal_nan=True)
        assert np.array_equal(d[:, 9:], h[:, 9:])
    assert hp.shape[0] > 1000 and hg.shape[0] > 500


def test_same_global_boxes_give_identical_matches_and_metrics(cuda):
    infos, results = nusc_samples(40, seed=32)
    tab, a = _encoded(infos, results)
    hp, hpc, hg, hgc = ne.host_global(a, tab)
    h = ne.host_core(hp, hpc, hg, hgc, tab)
    t = lambda x: torch.as_tensor(x, dtype=torch.float64, device=cuda).contiguous()   # noqa: E731
    d = ne.device_core(t(hp), offsets(hpc, cuda), t(hg), offsets(hgc, cuda), tab, ne._dev_tables(tab, cuda))
    assert np.array_equal(d["rank"], h["rank"]) and np.array_equal(d["cseg"], h["cseg"]) and np.array_equal(d["npos"], h["npos"])
    assert np.array_equal(d["tp"], h["tp"]) and np.array_equal(d["match"], h["match"])
    assert np.array_equal(d["mri"], h["mri"])
    for k in ("prec", "conf", "ap", "tp_err", "err"):
        assert np.abs(d[k] - h[k]).max() <= 1e-12, k
    assert h["tp"].sum() > 1000 and (h["ap"] > 0).all()


@pytest.mark.parametrize("seed", [33, 34])
def test_nuscenes_eval_device_matches_host(cuda, seed):
    infos, results = nusc_samples(60, preds_per_sample=80, seed=seed)
    got = ne.nuscenes_eval(results, infos, device=cuda, logger="silent")
    want = ne.nuscenes_eval(results, infos, device="cpu", logger="silent")
    _same(got, want)
    assert 0.1 < want[f"{P}/mAP"] < 0.9


def _empty():
    return dict(boxes_3d=np.zeros((0, 9), np.float32), scores_3d=np.zeros(0, np.float32), labels_3d=np.zeros(0, np.int64))


def test_streaming_batchings_are_bit_identical(cuda):
    infos, results = nusc_samples(30, seed=35)
    results = results[:5] + [_empty()] + results[6:]
    infos = infos[:9] + [dict(infos[9], gt_names=infos[9]["gt_names"][:0], gt_boxes=infos[9]["gt_boxes"][:0],
                              gt_velocity=infos[9]["gt_velocity"][:0], num_lidar_pts=infos[9]["num_lidar_pts"][:0],
                              num_radar_pts=infos[9]["num_radar_pts"][:0], gt_attr_names=infos[9]["gt_attr_names"][:0])] + infos[10:]
    outs = []
    for sizes in ([30], [1] * 30, [7, 0, 13, 10], [29, 1]):
        e = ne.NuScenesEvaluator(device=cuda)
        k = 0
        for n in sizes:
            e.add(results[k:k + n], infos[k:k + n])
            k += n
        assert len(e) == 30
        outs.append(e.compute())
    outs.append(e.compute())
    for o in outs[1:]:
        assert set(o) == set(outs[0])
        for key in o:
            assert np.float64(o[key]).tobytes() == np.float64(outs[0][key]).tobytes(), key
    _same(outs[0], ne.nuscenes_eval(results, infos, device=cuda, logger="silent"), tol=0.0)
    h = ne.NuScenesEvaluator(device="cpu")
    h.add(results, infos)
    _same(outs[0], h.compute())


def test_gt_as_predictions_on_device(cuda):
    infos, _ = nusc_samples(10, seed=36)
    results = [_gt_as_pred(i) for i in infos]
    r = ne.nuscenes_eval(results, infos, device=cuda, logger="silent")
    _same(r, ne.nuscenes_eval(results, infos, device="cpu", logger="silent"))
    assert all(r[f"{P}/{c}_AP_dist_{th}"] == 1.0 for c in ne.CLASSES for th in ne.DIST_THS)
    assert r[f"{P}/mATE"] == 0.0 and abs(r[f"{P}/NDS"] - 1.0) <= 1e-12


def test_errors_on_device(cuda):
    infos, results = nusc_samples(2, seed=37)
    bad = [dict(r, scores_3d=np.where(np.arange(len(r["scores_3d"])) == 0, np.nan, r["scores_3d"]).astype(np.float32)) for r in results]
    e = ne.NuScenesEvaluator(device=cuda)
    e.add(bad, infos)
    with pytest.raises(ValueError):
        e.compute()
    e = ne.NuScenesEvaluator(device=cuda)
    e.add([dict(r, labels_3d=np.full(len(r["labels_3d"]), 10)) for r in results], infos)
    with pytest.raises(ValueError):
        e.compute()
    many = dict(boxes_3d=np.zeros((501, 9), np.float32), scores_3d=np.zeros(501, np.float32), labels_3d=np.zeros(501, np.int64))
    with pytest.raises(ValueError):
        ne.NuScenesEvaluator(device=cuda).add([many], infos[:1])
    with pytest.raises(ValueError):
        ne.nuscenes_eval([many], infos[:1], device=cuda)
    with pytest.raises(ValueError):
        ne.nuscenes_eval([dict(results[0], labels_3d=results[0]["labels_3d"] + 10)], infos[:1], device=cuda)
    r = ne.nuscenes_eval([_empty(), _empty()], infos, device=cuda, logger="silent")
    assert r[f"{P}/mAP"] == 0.0 and r[f"{P}/car_trans_err"] == 1.0


def test_simple_test_results_evaluate_on_device_as_on_host(cuda):
    import ast
    import os

    import projects.mmdet3d_plugin  # noqa: F401
    from oracle.weights import seeded_tensor
    from uni3detr_amd.registry import build_model, to_config

    shipped = os.path.join(os.path.dirname(__file__), "golden", "shipped_configs.txt")
    model = build_model(to_config(ast.literal_eval(open(shipped).read())["nuscenes"]["config"]["model"]))
    model.load_state_dict({k: seeded_tensor(k, tuple(v.shape), 3) for k, v in model.state_dict().items()})
    model = model.to(cuda).eval()
    infos, _ = nusc_samples(2, seed=38)
    rng = np.random.default_rng(38)
    pts = [np.concatenate([rng.uniform((-54, -54, -5), (54, 54, 3), (30000, 3)), rng.uniform(0, 1, (30000, 2))], 1).astype(np.float32)
           for _ in infos]
    with torch.no_grad():
        res = model.simple_test(None, [torch.from_numpy(p).to(cuda) for p in pts])
    assert sum(len(r.get("pts_bbox", r)["scores_3d"]) for r in res) > 0
    dev, host = ne.NuScenesEvaluator(device=cuda), ne.NuScenesEvaluator(device="cpu")
    dev.add(res, infos)
    host.add(res, infos)
    _same(dev.compute(), host.compute())


def test_empty_first_middle_and_last_sample_change_nothing(cuda):
    """samples with neither predictions nor GT, in front of, between and behind two others: every box keeps its own sample's
    calibration and GT, so the result is that of the two samples alone, bit for bit"""
    infos, results = nusc_samples(2, seed=37)
    none = dict(infos[0], **{k: infos[0][k][:0] for k in ("gt_names", "gt_boxes", "gt_velocity", "num_lidar_pts", "num_radar_pts", "gt_attr_names")})
    outs = []
    for r, i in ((results, infos), ([_empty(), results[0], _empty(), results[1], _empty()], [none, infos[0], none, infos[1], none])):
        e = ne.NuScenesEvaluator(device=cuda)
        e.add(r, i)
        outs.append(e.compute())
    assert set(outs[0]) == set(outs[1]) and outs[0]["pts_bbox_NuScenes/mAP"] > 0
    for k in outs[0]:
        assert np.float64(outs[0][k]).tobytes() == np.float64(outs[1][k]).tobytes(), k
