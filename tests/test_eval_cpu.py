"""Indoor detection evaluation, host path (uni3detr_amd/evaluation.py, device="cpu"): anchored to the reference's own indoor_eval_ov
(loaded from where it lies, skipped where the reference tree is absent), to the oracle's rotated 3-D IoU, and to hand-computed cases."""
import importlib.util
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

from oracle import boxes as ob
from oracle.refshim import REF_ROOT
from uni3detr_amd import evaluation as ev
from uni3detr_amd.synth import eval_scenes

REF_EVAL = os.path.join(REF_ROOT, "projects", "mmdet3d_plugin", "core", "indoor_eval.py")
THRS = (0.25, 0.5)


class _DepthBoxes:
    """Stand-in for mmdet3d's DepthInstance3DBoxes: what the reference's indoor_eval touches, with the oracle's overlaps."""

    def __init__(self, tensor, box_dim=7, with_yaw=True, origin=(0.5, 0.5, 0)):
        t = torch.as_tensor(np.asarray(tensor) if not isinstance(tensor, torch.Tensor) else tensor, dtype=torch.float32)
        t = t.reshape(0, 7) if t.numel() == 0 else t.reshape(t.shape[0], -1)
        if t.shape[1] == 6:
            t = torch.cat([t, t.new_zeros(t.shape[0], 1)], 1)
        t = t.clone()
        if tuple(origin) != (0.5, 0.5, 0):
            t[:, :3] += t[:, 3:6] * (t.new_tensor((0.5, 0.5, 0)) - t.new_tensor(origin))
        self.tensor = t

    def __len__(self):
        return self.tensor.shape[0]

    def __getitem__(self, i):
        return _DepthBoxes(self.tensor[i].view(1, -1))

    def convert_to(self, mode):
        return self

    def new_box(self, data):
        return _DepthBoxes(data)

    @property
    def corners(self):
        t = self.tensor
        n = torch.tensor([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=torch.float32) - t.new_tensor((0.5, 0.5, 0))
        c = t[:, None, 3:6] * n[None]
        cs, sn = torch.cos(t[:, 6])[:, None], torch.sin(t[:, 6])[:, None]
        x, y = c[..., 0] * cs - c[..., 1] * sn, c[..., 0] * sn + c[..., 1] * cs
        return torch.stack([x, y, c[..., 2]], -1) + t[:, None, :3]

    @classmethod
    def overlaps(cls, b1, b2):
        return ob.bbox_overlaps_3d(b1.tensor, b2.tensor)


def _load_reference(monkeypatch):
    if not os.path.exists(REF_EVAL):
        pytest.skip("reference tree not available")
    mmcv, utils, tt = types.ModuleType("mmcv"), types.ModuleType("mmcv.utils"), types.ModuleType("terminaltables")
    utils.print_log = lambda msg, logger=None: None
    mmcv.utils = utils

    class AsciiTable:
        def __init__(self, data):
            self.table = "\n".join(" ".join(map(str, r)) for r in data)
    tt.AsciiTable = AsciiTable
    monkeypatch.setitem(sys.modules, "mmcv", mmcv)
    monkeypatch.setitem(sys.modules, "mmcv.utils", utils)
    monkeypatch.setitem(sys.modules, "terminaltables", tt)
    spec = importlib.util.spec_from_file_location("_ref_indoor_eval", REF_EVAL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _margin_keep(gt, gl, db, dl, thrs, axis_aligned_lw):
    """False for a detection whose float64 iou_max lies within 1e-4 of a threshold, or whose top-two IoUs lie within 1e-6 of each
    other while its best IoU can still match (the outcome would hinge on rounding)."""
    g = ev._gt_bottom_boxes(gt, axis_aligned_lw)
    keep = np.ones(len(dl), bool)
    for i in range(len(dl)):
        sel = gl == dl[i]
        if not sel.any():
            continue
        v = np.sort(ev.bbox_overlaps_3d(db[i:i + 1], g[sel])[0])[::-1]
        if any(abs(v[0] - t) < 1e-4 for t in thrs):
            keep[i] = False
        if len(v) > 1 and v[0] > min(thrs) - 1e-4 and v[0] - v[1] < 1e-6:
            keep[i] = False
    return keep


def _dataset(seed=0, n_scenes=40, num_classes=6):
    rng = np.random.default_rng(seed + 100)
    sc = eval_scenes(n_scenes, rng.integers(0, 30, n_scenes), num_classes, seed=seed, max_gt=6, tp_frac=0.5, dup=3)
    out = []
    for s, (gt, gl, db, ds, dl) in enumerate(sc):
        if s in (3, 7):                                            # scenes without GT
            gt, gl = gt[:0], gl[:0]
        if s in (5, 11):                                           # scenes without detections
            db, ds, dl = db[:0], ds[:0], dl[:0]
        keep = dl != 4                                             # class 4: GT only
        db, ds, dl = db[keep], ds[keep], dl[keep]
        gk = gl != 5                                               # class 5: predictions only
        gt, gl = gt[gk], gl[gk]
        keep = _margin_keep(gt, gl, db, dl, THRS, False) & _margin_keep(gt, gl, db, dl, THRS, True)
        out.append([gt, gl, db[keep], ds[keep], dl[keep]])
    n = sum(len(x[4]) for x in out)
    scores = rng.permutation(np.linspace(0.05, 0.95, n).astype(np.float32))         # distinct: the reference's order is unambiguous
    k = 0
    for x in out:
        x[3] = scores[k:k + len(x[4])]
        k += len(x[4])
    return out


def _annos(data, box_cls=None):
    gt_annos, dt_annos = [], []
    for gt, gl, db, ds, dl in data:
        gt_annos.append(dict(gt_num=len(gl), gt_boxes_upright_depth=gt.copy(), **{"class": gl.copy()}))
        b = torch.from_numpy(db.copy()).reshape(-1, 7)
        dt_annos.append(dict(boxes_3d=box_cls(b) if box_cls else b, scores_3d=torch.from_numpy(ds.copy()),
                             labels_3d=torch.from_numpy(dl.copy())))
    return gt_annos, dt_annos


def _assert_same(got, want, tol=1e-6):
    assert set(got) == set(want), set(got) ^ set(want)
    for k in want:
        a, b = got[k], want[k]
        assert math.isnan(a) == math.isnan(b), (k, a, b)
        if not math.isnan(b):
            assert abs(a - b) <= tol, (k, a, b)


@pytest.mark.parametrize("axis_aligned_lw", [False, True])
def test_host_path_matches_reference_indoor_eval(monkeypatch, axis_aligned_lw):
    ref = _load_reference(monkeypatch)
    data = _dataset()
    label2cat = {i: f"c{i}" for i in range(6)}
    g1, d1 = _annos(data, _DepthBoxes)
    want = ref.indoor_eval_ov(list(label2cat.values()), g1, d1, THRS, label2cat, box_type_3d=_DepthBoxes, box_mode_3d=None,
                              axis_aligned_lw=axis_aligned_lw)
    g2, d2 = _annos(data)
    got = ev.indoor_eval(g2, d2, THRS, label2cat, logger="silent", axis_aligned_lw=axis_aligned_lw, device="cpu")
    _assert_same(got, want)
    # the edge cases are really in the data: GT-only class -> 0, prediction-only class -> NaN, and something is matched
    assert want["c4_AP_0.25"] == 0.0 and want["c4_rec_0.25"] == 0.0
    assert math.isnan(want["c5_AP_0.25"]) and math.isnan(want["c5_rec_0.50"])
    assert 0.0 < want["mAP_0.25"] < 1.0 and 0.0 < want["mAR_0.50"] < 1.0
    # the ov wrapper returns the same dict
    _assert_same(ev.indoor_eval_ov(list(label2cat.values()), g2, d2, THRS, label2cat, logger="silent", axis_aligned_lw=axis_aligned_lw,
                                   device="cpu"), want)


def test_host_iou_matches_oracle():
    rng = np.random.default_rng(7)
    n = 400
    a = np.concatenate([rng.uniform(-2, 2, (n, 3)), rng.uniform(0.2, 2.0, (n, 3)), rng.uniform(-np.pi, np.pi, (n, 1))], 1)
    b = a + np.concatenate([rng.normal(0, 0.3, (n, 3)), rng.normal(0, 0.2, (n, 3)), rng.normal(0, 0.5, (n, 1))], 1)
    b[:, 3:6] = np.abs(b[:, 3:6]) + 0.05
    b[:50, 3] = 1e-6                                              # widths below the 1e-4 clamp
    b[50:100] = a[50:100]                                         # identical boxes
    b[100:150, :2] += 10.0                                        # disjoint
    got = ev.box_iou3d_pairs(a, b)
    want = ob.bbox_overlaps_3d_aligned(torch.from_numpy(a), torch.from_numpy(b)).numpy()
    assert np.abs(got - want).max() <= 1e-9
    assert np.allclose(got[50:100], 1.0) and np.all(got[100:150] == 0.0)
    m = ev.bbox_overlaps_3d(a[:20], b[:30])
    assert np.abs(m - ob.bbox_overlaps_3d(torch.from_numpy(a[:20]), torch.from_numpy(b[:30])).numpy()).max() <= 1e-9


def _box(x, y, z=0.0, d=1.0, yaw=0.0):
    return [x, y, z, d, d, d, yaw]


def _flat(det, gt, thrs=(0.25, 0.5)):
    """det / gt: per scene lists of (box, score, label) / (box, label), bottom-centre boxes."""
    db = np.array([b for s in det for b, _, _ in s], np.float32).reshape(-1, 7)
    ds = np.array([c for s in det for _, c, _ in s], np.float32)
    dl = np.array([c for s in det for _, _, c in s], np.int64)
    gb = np.array([b for s in gt for b, _ in s], np.float32).reshape(-1, 7)
    gl = np.array([c for s in gt for _, c in s], np.int64)
    return ev.evaluate_flat(db, ds, dl, [len(s) for s in det], gb, gl, [len(s) for s in gt], 3, thrs, "cpu")


def test_hand_computed_ap():
    g0, g1 = _box(0, 0), _box(5, 0)
    r = _flat([[(g0, 0.9, 0), (g0, 0.8, 0), (g1, 0.7, 0)]], [[(g0, 0), (g1, 0)]])
    # TP, duplicate (FP), TP: recall .5 .5 1, precision 1 .5 2/3 -> AP = .5 * 1 + .5 * 2/3
    assert r["tp"].tolist() == [[1, 0, 1], [1, 0, 1]]
    assert r["ap"][0, 0] == np.float32(0.5 + 0.5 * 2.0 / 3.0) and r["rec"][0, 0] == 1.0
    # first maximal GT wins: two identical GT, the detection takes the first
    r = _flat([[(g0, 0.9, 1)]], [[(g1, 1), (g0, 1), (g0, 1)]])
    assert r["jmax"].tolist() == [1]
    # a detection of a class without GT anywhere: NaN; a class with GT and no detections: 0; the mean skips the NaN
    gt_annos = [dict(gt_num=1, gt_boxes_upright_depth=np.array([[0, 0, 0.5, 1, 1, 1, 0]], np.float32), **{"class": np.array([0])})]
    dt_annos = [dict(boxes_3d=torch.tensor([g0, g0]), scores_3d=torch.tensor([0.9, 0.8]), labels_3d=torch.tensor([0, 2]))]
    out = ev.indoor_eval(gt_annos, dt_annos, (0.25,), {0: "a", 1: "b", 2: "c"}, logger="silent", device="cpu")
    assert out["a_AP_0.25"] == 1.0 and math.isnan(out["c_AP_0.25"]) and math.isnan(out["c_rec_0.25"]) and "b_AP_0.25" not in out
    assert out["mAP_0.25"] == 1.0 and out["mAR_0.25"] == 1.0
    # no predictions at all is not an error
    out = ev.indoor_eval(gt_annos, [dict(boxes_3d=torch.zeros(0, 7), scores_3d=torch.zeros(0), labels_3d=torch.zeros(0, dtype=torch.long))],
                         (0.25,), {0: "a"}, logger="silent", device="cpu")
    assert out == {"a_AP_0.25": 0.0, "mAP_0.25": 0.0, "a_rec_0.25": 0.0, "mAR_0.25": 0.0}


def test_ties_are_stable_by_scene_then_position():
    g0 = _box(0, 0)
    far = _box(9, 9)
    # equal scores: the FP of scene 0 ranks before the TP of scene 1 -> precision 1/2 at the only recall step
    r = _flat([[(far, 0.5, 0)], [(g0, 0.5, 0)]], [[], [(g0, 0)]])
    assert r["order"].tolist() == [0, 1] and r["ap"][0, 0] == np.float32(0.5)
    r = _flat([[(g0, 0.5, 0)], [(far, 0.5, 0)]], [[(g0, 0)], []])
    assert r["ap"][0, 0] == np.float32(1.0)
    # inside one scene: list position
    r = _flat([[(far, 0.5, 0), (g0, 0.5, 0)]], [[(g0, 0)]])
    assert r["order"].tolist() == [0, 1] and r["ap"][0, 0] == np.float32(0.5)


def test_non_finite_scores_raise():
    g0 = _box(0, 0)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            _flat([[(g0, bad, 0)]], [[(g0, 0)]])


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


def _assert_bitwise(a, b):
    assert set(a) == set(b), set(a) ^ set(b)
    for k in a:
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (k, a[k], b[k])


def test_streaming_evaluator_is_batch_independent_on_host():
    data = _with_empty_scenes(eval_scenes(12, 20, 4, seed=3))
    full = None
    for bs in (1, 5, 12):
        e = ev.IndoorEvaluator(4, device="cpu")
        for s in range(0, len(data), bs):
            chunk = data[s:s + bs]
            e.add([[torch.from_numpy(d[2]), torch.from_numpy(d[3]), torch.from_numpy(d[4])] for d in chunk],
                  [torch.from_numpy(d[0]) for d in chunk], [torch.from_numpy(d[1]) for d in chunk])
        out = e.compute()
        if full is not None:
            _assert_bitwise(out, full)
        full = out
    # the evaluator and indoor_eval agree
    ga, da = _annos([list(d) for d in data])
    _assert_same(ev.indoor_eval(ga, da, (0.25, 0.5), {c: str(c) for c in range(4)}, logger="silent", device="cpu"), full, tol=0.0)


def test_evaluator_accepts_a_scene_without_detections():
    gt = torch.tensor([[0.0, 0.0, 0.5, 1.0, 1.0, 1.0, 0.0]])
    e = ev.IndoorEvaluator(3, device="cpu")
    e.add([[torch.zeros(0, 7), torch.zeros(0), torch.zeros(0, dtype=torch.long)]], [gt], [torch.tensor([1])])
    e.add([dict(boxes_3d=torch.zeros(0, 9), scores_3d=torch.zeros(0), labels_3d=torch.zeros(0, dtype=torch.long))], [gt[:0]],
          [torch.zeros(0, dtype=torch.long)])
    out = e.compute()
    assert out == {"1_AP_0.25": 0.0, "mAP_0.25": 0.0, "1_rec_0.25": 0.0, "mAR_0.25": 0.0,
                   "1_AP_0.50": 0.0, "mAP_0.50": 0.0, "1_rec_0.50": 0.0, "mAR_0.50": 0.0}


def test_evaluator_rejects_labels_outside_num_classes_on_host():
    g0 = torch.tensor([[0.0, 0.0, 0.5, 1.0, 1.0, 1.0, 0.0]])
    for det_label, gt_label in ((3, 0), (0, 3)):
        e = ev.IndoorEvaluator(3, device="cpu")
        e.add([[g0, torch.tensor([0.9]), torch.tensor([det_label])]], [g0], [torch.tensor([gt_label])])
        with pytest.raises(ValueError):
            e.compute()


def test_no_scenes_on_host():
    out = ev.indoor_eval([], [], (0.25, 0.5), {0: "a"}, logger="silent", device="cpu")
    assert set(out) == {"mAP_0.25", "mAR_0.25", "mAP_0.50", "mAR_0.50"} and all(math.isnan(v) for v in out.values())
