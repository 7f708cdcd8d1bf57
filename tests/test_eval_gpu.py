"""Indoor detection evaluation on the device (csrc/eval.hip through uni3detr_amd/evaluation.py) against the float64 host path."""
import math

import numpy as np
import pytest
import torch

from uni3detr_amd import evaluation as ev
from uni3detr_amd.synth import eval_scenes, room_scene

pytestmark = pytest.mark.gpu
THRS = (0.25, 0.5)


def _flat(data):
    gb = np.concatenate([ev._gt_bottom_boxes(d[0]) for d in data])
    gl = np.concatenate([d[1] for d in data])
    db = np.concatenate([d[2] for d in data])
    ds = np.concatenate([d[3] for d in data])
    dl = np.concatenate([d[4] for d in data])
    return db, ds, dl, [len(d[4]) for d in data], gb, gl, [len(d[1]) for d in data]


def _margin_filter(data, thrs=THRS):
    """drop detections whose float64 iou_max lies within 1e-4 of a threshold or whose top-two IoUs are within 1e-5 while it can match."""
    out = []
    for gt, gl, db, ds, dl in data:
        g = ev._gt_bottom_boxes(gt)
        keep = np.ones(len(dl), bool)
        for c in np.unique(dl):
            sel, gs = np.nonzero(dl == c)[0], gl == c
            if not gs.any():
                continue
            v = -np.sort(-ev.bbox_overlaps_3d(db[sel], g[gs]), 1)
            bad = np.zeros(len(sel), bool)
            for t in thrs:
                bad |= np.abs(v[:, 0] - t) < 1e-4
            if v.shape[1] > 1:
                bad |= (v[:, 0] > min(thrs) - 1e-4) & (v[:, 0] - v[:, 1] < 1e-5)
            keep[sel[bad]] = False
        out.append((gt, gl, db[keep], ds[keep], dl[keep]))
    return out


def _same(got, want, tol=1e-6):
    assert set(got) == set(want), set(got) ^ set(want)
    for k in want:
        assert math.isnan(got[k]) == math.isnan(want[k]), k
        if not math.isnan(want[k]):
            assert abs(got[k] - want[k]) <= tol, (k, got[k], want[k])


def _annos(data):
    ga = [dict(gt_num=len(d[1]), gt_boxes_upright_depth=d[0], **{"class": d[1]}) for d in data]
    da = [dict(boxes_3d=torch.from_numpy(d[2]), scores_3d=torch.from_numpy(d[3]), labels_3d=torch.from_numpy(d[4])) for d in data]
    return ga, da


def test_iou_argmax_matches_float64_oracle(cuda):
    data = eval_scenes(24, 300, 5, seed=11)
    db, ds, dl, dc, gb, gl, gc = _flat(data)
    d = ev.evaluate_flat(db, ds, dl, dc, gb, gl, gc, 5, THRS, cuda)
    h = ev.evaluate_flat(db, ds, dl, dc, gb, gl, gc, 5, THRS, "cpu")
    im, jm = d["iou_max"].cpu().numpy().astype(np.float64), d["jmax"].cpu().numpy()
    has = h["jmax"] >= 0
    assert np.array_equal(jm >= 0, has) and np.all(np.isneginf(im[~has]))
    assert np.abs(im[has] - h["iou_max"][has]).max() <= 1e-5
    assert (h["iou_max"][has] > 0.25).sum() > 100                 # real matches are exercised
    # jmax identical wherever the best two same-class GT are more than 1e-5 apart
    off = np.concatenate([[0], np.cumsum(gc)])
    det_scene = np.repeat(np.arange(len(dc)), dc)
    checked = 0
    for i in np.nonzero(has)[0]:
        s = det_scene[i]
        idx = np.arange(off[s], off[s + 1])[gl[off[s]:off[s + 1]] == dl[i]]
        v = np.sort(ev.bbox_overlaps_3d(db[i:i + 1], gb[idx])[0])[::-1]
        if len(v) == 1 or v[0] - v[1] > 1e-5:
            assert jm[i] == h["jmax"][i], i
            checked += 1
    assert checked > 1000                 # (detections whose same-class GT all have IoU 0 tie at the top and are not checked)


def test_tp_flags_and_ap_match_host_fed_device_matches(cuda):
    data = eval_scenes(32, 400, 6, seed=12)
    db, ds, dl, dc, gb, gl, gc = _flat(data)
    d = ev.evaluate_flat(db, ds, dl, dc, gb, gl, gc, 6, THRS, cuda)
    im, jm = d["iou_max"].cpu().numpy(), d["jmax"].cpu().numpy()
    order = ev.host_rank(ds, dl)
    assert np.array_equal(d["perm"].cpu().numpy(), order)
    tp = ev.host_tp(order, im, jm, THRS)
    assert np.array_equal(d["tp"].cpu().numpy(), tp)
    assert tp.sum() > 50
    npos = np.bincount(gl, minlength=6)
    ap, rec = ev.host_ap(tp, dl[order], npos, 6)
    assert np.array_equal(np.isnan(ap), np.isnan(d["ap"])) and np.nanmax(np.abs(ap - d["ap"])) <= 1e-6
    assert np.nanmax(np.abs(rec - d["rec"])) <= 1e-12


@pytest.mark.parametrize("shape", [(64, 1000, 10, 21), (16, 5000, 18, 22)], ids=["sunrgbd", "scannet"])
def test_device_indoor_eval_matches_host(cuda, shape):
    n_scenes, n_det, ncls, seed = shape
    data = _margin_filter(eval_scenes(n_scenes, n_det, ncls, seed=seed, max_gt=30 if ncls == 18 else 12))
    label2cat = {c: f"cls{c}" for c in range(ncls)}
    ga, da = _annos(data)
    want = ev.indoor_eval(ga, da, THRS, label2cat, logger="silent", device="cpu")
    got = ev.indoor_eval(ga, da, THRS, label2cat, logger="silent", device=cuda)
    _same(got, want)
    assert 0.0 < want["mAP_0.25"] < 1.0
    e = ev.IndoorEvaluator(ncls, THRS, device=cuda)
    e.add([[torch.from_numpy(d[2]).to(cuda), torch.from_numpy(d[3]).to(cuda), torch.from_numpy(d[4]).to(cuda)] for d in data],
          [torch.from_numpy(d[0]).to(cuda) for d in data], [torch.from_numpy(d[1]).to(cuda) for d in data])
    _same(e.compute(label2cat), want)


def test_ties_follow_the_stable_host_order(cuda):
    data = eval_scenes(16, 200, 4, seed=13)
    data = [(g, l, b, np.round(s * 4) / 4, c) for g, l, b, s, c in data]       # five score values: ties everywhere
    data = [(g, l, b, s.astype(np.float32), c) for g, l, b, s, c in data]
    db, ds, dl, dc, gb, gl, gc = _flat(data)
    d = ev.evaluate_flat(db, ds, dl, dc, gb, gl, gc, 4, THRS, cuda)
    assert np.array_equal(d["perm"].cpu().numpy(), ev.host_rank(ds, dl))
    ga, da = _annos(_margin_filter(data))
    _same(ev.indoor_eval(ga, da, THRS, {c: str(c) for c in range(4)}, logger="silent", device=cuda),
          ev.indoor_eval(ga, da, THRS, {c: str(c) for c in range(4)}, logger="silent", device="cpu"))


def _with_empty_scenes(data):
    """scenes 2 and 6 without detections (what get_bboxes returns after its range / score filters), scene 4 without GT"""
    out = []
    for s, (gt, gl, db, ds, dl) in enumerate(data):
        if s in (2, 6):
            db, ds, dl = db[:0], ds[:0], dl[:0]
        if s == 4:
            gt, gl = gt[:0], gl[:0]
        out.append((gt, gl, db, ds, dl))
    return out


def test_streaming_batches_are_bit_identical(cuda):
    data = _with_empty_scenes(eval_scenes(64, 150, 5, seed=14))
    outs = []
    for bs in (64, 1, 8, 64):
        e = ev.IndoorEvaluator(5, THRS, device=cuda)
        for s in range(0, len(data), bs):
            ch = data[s:s + bs]
            e.add([[torch.from_numpy(d[2]).to(cuda), torch.from_numpy(d[3]).to(cuda), torch.from_numpy(d[4]).to(cuda)] for d in ch],
                  [torch.from_numpy(d[0]).to(cuda) for d in ch], [torch.from_numpy(d[1]).to(cuda) for d in ch])
        outs.append(e.compute())
    for o in outs[1:]:
        assert set(o) == set(outs[0])
        for k in o:
            assert np.float64(o[k]).tobytes() == np.float64(outs[0][k]).tobytes(), k
    # ... and equal to indoor_eval over the same scenes (including those without detections / GT), on the device and on the host
    ga, da = _annos(_margin_filter(data))
    label2cat = {c: str(c) for c in range(5)}
    e = ev.IndoorEvaluator(5, THRS, device=cuda)
    e.add([[torch.from_numpy(d["boxes_3d"].numpy()).to(cuda), d["scores_3d"].to(cuda), d["labels_3d"].to(cuda)] for d in da],
          [torch.from_numpy(g["gt_boxes_upright_depth"]).to(cuda) for g in ga], [torch.from_numpy(g["class"]).to(cuda) for g in ga])
    got = e.compute(label2cat)
    _same(got, ev.indoor_eval(ga, da, THRS, label2cat, logger="silent", device=cuda), tol=0.0)
    _same(got, ev.indoor_eval(ga, da, THRS, label2cat, logger="silent", device="cpu"))


def test_evaluator_rejects_labels_outside_num_classes_on_device(cuda):
    g0 = torch.tensor([[0.0, 0.0, 0.5, 1.0, 1.0, 1.0, 0.0]], device=cuda)
    for det_label, gt_label in ((3, 0), (0, 3)):
        e = ev.IndoorEvaluator(3, THRS, device=cuda)
        e.add([[g0, torch.tensor([0.9], device=cuda), torch.tensor([det_label], device=cuda)]], [g0], [torch.tensor([gt_label], device=cuda)])
        with pytest.raises(ValueError):
            e.compute()


def test_no_scenes_on_device(cuda):
    out = ev.indoor_eval([], [], THRS, {0: "a"}, logger="silent", device=cuda)
    assert set(out) == {"mAP_0.25", "mAR_0.25", "mAP_0.50", "mAR_0.50"} and all(math.isnan(v) for v in out.values())


def test_gt_as_predictions_is_perfect(cuda):
    data = eval_scenes(20, 10, 6, seed=15)
    e = ev.IndoorEvaluator(6, THRS, device=cuda)
    bl = []
    for gt, gl, *_ in data:
        b = torch.from_numpy(ev._gt_bottom_boxes(gt)).to(cuda)
        bl.append([b, torch.rand(len(gl), device=cuda), torch.from_numpy(gl).to(cuda)])
    e.add(bl, [torch.from_numpy(d[0]).to(cuda) for d in data], [torch.from_numpy(d[1]).to(cuda) for d in data])
    out = e.compute()
    present = {int(c) for d in data for c in d[1]}
    assert present
    for c in present:
        for t in ("0.25", "0.50"):
            assert out[f"{c}_AP_{t}"] == 1.0 and out[f"{c}_rec_{t}"] == 1.0


def test_simple_test_results_evaluate_on_device_as_on_host(cuda):
    import projects.mmdet3d_plugin  # noqa: F401
    from oracle.weights import seeded_tensor
    from uni3detr_amd.configs.sunrgbd import model as MODEL_CFG
    from uni3detr_amd.registry import build_model

    model = build_model(MODEL_CFG)
    model.load_state_dict({k: seeded_tensor(k, tuple(v.shape), 3) for k, v in model.state_dict().items()})
    model = model.to(cuda).eval()
    scenes = [room_scene(i, 6000) for i in range(2)]
    res = model.simple_test(None, [torch.from_numpy(p).to(cuda) for p, _, _ in scenes])
    assert sum(len(r["scores_3d"]) for r in res) > 0
    ga = [dict(gt_num=len(lab), gt_boxes_upright_depth=gt, **{"class": lab}) for _, gt, lab in scenes]
    label2cat = {c: str(c) for c in range(10)}
    _same(ev.indoor_eval(ga, res, THRS, label2cat, logger="silent", device=cuda),
          ev.indoor_eval(ga, res, THRS, label2cat, logger="silent", device="cpu"))


def test_empty_first_middle_and_last_scene_change_nothing(cuda):
    """scenes with neither detections nor GT, in front of, between and behind two others: every detection still meets the GT of its own
    scene, so the result is that of the two scenes alone, bit for bit"""
    data = eval_scenes(2, 140, 5, seed=19)
    none = tuple(x[:0] for x in data[0])
    outs = []
    for scenes in (data, [none, data[0], none, data[1], none]):
        e = ev.IndoorEvaluator(5, THRS, device=cuda)
        e.add([[torch.from_numpy(d[2]).to(cuda), torch.from_numpy(d[3]).to(cuda), torch.from_numpy(d[4]).to(cuda)] for d in scenes],
              [torch.from_numpy(d[0]).to(cuda) for d in scenes], [torch.from_numpy(d[1]).to(cuda) for d in scenes])
        outs.append(e.compute())
    assert set(outs[0]) == set(outs[1]) and 0.0 < outs[0]["mAP_0.25"] <= 1.0
    for k in outs[0]:
        assert np.float64(outs[0][k]).tobytes() == np.float64(outs[1][k]).tobytes(), k
