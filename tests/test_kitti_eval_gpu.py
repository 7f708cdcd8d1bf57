"""KITTI detection evaluation on the device (csrc/kitti_eval.hip through uni3detr_amd/kitti_eval.py) against the float64 host path."""
import numpy as np
import pytest
import torch

from uni3detr_amd import kitti_eval as ke
from uni3detr_amd.synth import kitti_scenes

pytestmark = pytest.mark.gpu
CLASSES = ["Pedestrian", "Cyclist", "Car"]
THRS = (0.25, 0.5, 0.7)


def _f32(annos):
    """round every float field to float32: both paths then read the same numbers"""
    out = []
    for a in annos:
        b = dict(a)
        for k in ("bbox", "location", "dimensions", "rotation_y", "alpha", "score", "truncated"):
            if k in b:
                b[k] = np.asarray(b[k], np.float32).astype(np.float64)
        out.append(b)
    return out


def _data(n, seed, det_per_scene=40):
    infos, results = kitti_scenes(n, det_per_scene=det_per_scene, seed=seed)
    gt = _f32([i["annos"] for i in infos])
    dt = _f32(ke.lidar_results_to_kitti(results, infos, CLASSES))
    return infos, results, gt, dt


def _margin_filter(gt_annos, dt_annos):
    """drop detections with an overlap (any metric, any GT) or a DontCare IoF within 1e-4 of a threshold"""
    out = []
    for g, d in zip(gt_annos, dt_annos):
        gr, dr = ke._encode(g, True), ke._encode(d, False)
        bad = np.zeros(dr.shape[0], bool)
        if gr.shape[0] and dr.shape[0]:
            ov = ke.scene_overlaps(dr, gr)
            dcf = ke.dc_iof(dr, gr)
            for t in THRS:
                bad |= (np.abs(ov - t) < 1e-4).any(axis=(0, 2)) | (np.abs(dcf - t) < 1e-4)
        out.append({k: (v[~bad] if isinstance(v, np.ndarray) and v.shape[:1] == bad.shape else v) for k, v in d.items()})
    return out


def _same(got, want, tol=0.0):
    assert set(got) == set(want), set(got) ^ set(want)
    for k in want:
        assert abs(got[k] - want[k]) <= tol, (k, got[k], want[k])


def test_device_overlaps_match_float64_host(cuda):
    _, _, gt, dt = _data(40, seed=1)
    g, gc = ke._encode_all(gt, True)
    d, dc = ke._encode_all(dt, False)
    r = ke.evaluate_records(d, dc, g, gc, [0, 1, 2], [0, 1, 2], True, cuda)
    ov = r["ov"].cpu().numpy().astype(np.float64)
    off = r["ov_off"].cpu().numpy()
    doff, goff = np.concatenate([[0], np.cumsum(dc)]), np.concatenate([[0], np.cumsum(gc)])
    pairs, hits = 0, 0
    for s in range(len(dc)):
        want = ke.scene_overlaps(d[doff[s]:doff[s + 1]], g[goff[s]:goff[s + 1]])
        got = ov[:, off[s]:off[s + 1]].reshape(want.shape)
        assert np.abs(got - want).max(initial=0.0) <= 1e-5, s
        pairs += want[0].size
        hits += int((want > 0.5).sum())
        dcf = ke.dc_iof(d[doff[s]:doff[s + 1]], g[goff[s]:goff[s + 1]])
        assert np.abs(r["dc_iof"][doff[s]:doff[s + 1]].cpu().numpy() - dcf).max(initial=0.0) <= 1e-5
    assert pairs > 5000 and hits > 200


def test_same_overlaps_give_identical_flags_thresholds_counts_and_ap(cuda):
    _, _, gt, dt = _data(60, seed=2)
    g, gc = ke._encode_all(gt, True)
    d, dc = ke._encode_all(dt, False)
    d32, g32 = d.astype(np.float32).astype(np.float64), g.astype(np.float32).astype(np.float64)
    r = ke.evaluate_records(d32, dc, g32, gc, [0, 1, 2], [0, 1, 2], True, cuda)
    ov = r["ov"].cpu().numpy().astype(np.float64)
    off = r["ov_off"].cpu().numpy()
    doff = np.concatenate([[0], np.cumsum(dc)])
    ovs = [ov[:, off[s]:off[s + 1]].reshape(3, dc[s], gc[s]) for s in range(len(dc))]
    dcf = r["dc_iof"].cpu().numpy().astype(np.float64)
    h = ke.host_core(d32, dc, g32, gc, [0, 1, 2], [0, 1, 2], True, ov=ovs, dcf=[dcf[doff[s]:doff[s + 1]] for s in range(len(dc))])
    assert np.array_equal(r["gt_flag"].cpu().numpy(), h["gt_flag"]) and np.array_equal(r["dt_flag"].cpu().numpy(), h["dt_flag"])
    assert np.array_equal(r["nvalid"].cpu().numpy(), h["nvalid"])
    assert np.array_equal(r["nthr"].cpu().numpy(), h["nthr"])
    assert np.array_equal(r["thr"].cpu().numpy().astype(np.float64), h["thr"])
    assert np.array_equal(r["tot"].cpu().numpy(), h["tot"])
    assert np.array_equal(r["ap"][:, :2], h["ap"][:, :2])                    # 2-D / BEV / 3-D AP: bit-identical
    assert np.abs(r["ap"][:, 2:] - h["ap"][:, 2:]).max() <= 1e-9             # AOS: device cos vs NumPy cos
    assert h["nthr"].sum() > 300 and h["tot"][:, 0].sum() > 1000


@pytest.mark.parametrize("seed", [3, 4])
def test_kitti_eval_device_matches_host(cuda, seed):
    _, _, gt, dt = _data(80, seed=seed, det_per_scene=60)
    dt = _margin_filter(gt, dt)
    s_dev, got = ke.kitti_eval(gt, dt, CLASSES, device=cuda)
    s_host, want = ke.kitti_eval(gt, dt, CLASSES, device="cpu")
    _same(got, want, tol=1e-9)
    assert "KITTI/Overall_AOS_AP40_moderate" in want and 0.0 < want["KITTI/Car_3D_AP40_moderate_strict"] < 100.0
    assert s_dev.splitlines()[:3] == s_host.splitlines()[:3]


def _empty_result():
    return dict(boxes_3d=np.zeros((0, 7), np.float32), scores_3d=np.zeros(0, np.float32), labels_3d=np.zeros(0, np.int64))


def test_streaming_batchings_are_bit_identical(cuda):
    infos, results, _, _ = _data(30, seed=5)
    infos = infos[:10] + [dict(infos[10], annos={k: v[:0] for k, v in infos[10]["annos"].items()})] + infos[11:]
    results = results[:5] + [_empty_result()] + results[6:]
    outs = []
    for sizes in ([30], [1] * 30, [7, 0, 13, 10], [29, 1]):
        e = ke.KittiEvaluator(CLASSES, device=cuda)
        k = 0
        for n in sizes:
            e.add(results[k:k + n], infos[k:k + n])
            k += n
        outs.append(e.compute())
    outs.append(e.compute())                                       # twice in a row
    for o in outs[1:]:
        assert set(o) == set(outs[0])
        for key in o:
            assert np.float64(o[key]).tobytes() == np.float64(outs[0][key]).tobytes(), key
    e = ke.KittiEvaluator(CLASSES, device="cpu")
    e.add(results, infos)
    _same(outs[0], e.compute(), tol=1e-6)


def test_gt_as_predictions_on_device(cuda):
    infos, _ = kitti_scenes(40, seed=6)
    gt = _f32([i["annos"] for i in infos])
    rng = np.random.default_rng(0)
    dt = [dict(a, score=rng.permutation(len(a["name"])).astype(np.float64) / 64 + 0.25) for a in gt]
    _, got = ke.kitti_eval(gt, dt, CLASSES, device=cuda)
    _, want = ke.kitti_eval(gt, dt, CLASSES, device="cpu")
    _same(got, want, tol=1e-9)
    assert got["KITTI/Car_3D_AP40_moderate_strict"] > 90.0


def test_errors_on_device(cuda):
    infos, results = kitti_scenes(2, seed=7)
    bad = [dict(r, scores_3d=np.where(np.arange(len(r["scores_3d"])) == 0, np.nan, r["scores_3d"]).astype(np.float32)) for r in results]
    e = ke.KittiEvaluator(CLASSES, device=cuda)
    e.add(bad, infos)
    with pytest.raises(ValueError):
        e.compute()
    with pytest.raises(ValueError):
        ke.KittiEvaluator(["Car", "Van"], device=cuda)
    _, r = ke.kitti_eval([i["annos"] for i in infos], [ke._empty_anno(None)] * 2, CLASSES, device=cuda)
    assert all(v == 0.0 for v in r.values())


def test_simple_test_results_evaluate_on_device_as_on_host(cuda):
    import ast
    import os

    import projects.mmdet3d_plugin  # noqa: F401
    from oracle.weights import seeded_tensor
    from uni3detr_amd.registry import build_model, to_config

    shipped = os.path.join(os.path.dirname(__file__), "golden", "shipped_configs.txt")
    model = build_model(to_config(ast.literal_eval(open(shipped).read())["kitti_3classes"]["config"]["model"]))
    model.load_state_dict({k: seeded_tensor(k, tuple(v.shape), 3) for k, v in model.state_dict().items()})
    model = model.to(cuda).eval()
    infos, _ = kitti_scenes(3, seed=8)
    rng = np.random.default_rng(8)
    pts = [np.concatenate([rng.uniform((0, -40, -3), (70.4, 40, 1), (16000, 3)), rng.uniform(0, 1, (16000, 1))], 1).astype(np.float32)
           for _ in infos]
    res = model.simple_test(None, [torch.from_numpy(p).to(cuda) for p in pts])
    assert sum(len(r["scores_3d"]) for r in res) > 0
    dev, host = ke.KittiEvaluator(CLASSES, device=cuda), ke.KittiEvaluator(CLASSES, device="cpu")
    dev.add(res, infos)
    host.add(res, infos)
    _same(dev.compute(), host.compute(), tol=1e-6)


def test_empty_first_middle_and_last_scene_change_nothing(cuda):
    """scenes with neither detections nor GT, in front of, between and behind two others: every detection keeps its own scene's
    calibration and GT, so the result is that of the two scenes alone, bit for bit"""
    infos, results = kitti_scenes(2, det_per_scene=40, seed=15)
    none = dict(infos[0], annos={k: v[:0] for k, v in infos[0]["annos"].items()})
    outs = []
    for r, i in ((results, infos), ([_empty_result(), results[0], _empty_result(), results[1], _empty_result()],
                                    [none, infos[0], none, infos[1], none])):
        e = ke.KittiEvaluator(CLASSES, device=cuda)
        e.add(r, i)
        outs.append(e.compute())
    assert set(outs[0]) == set(outs[1]) and any(v > 0 for v in outs[0].values())
    for k in outs[0]:
        assert np.float64(outs[0][k]).tobytes() == np.float64(outs[1][k]).tobytes(), k
