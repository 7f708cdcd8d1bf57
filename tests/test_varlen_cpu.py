"""Capacity-mode training step, host side: the point-capacity planner and the NumPy restatement of the batch ingest
(tests/ingest_ref.py) against hand-written cases and against Uni3DETRHead._pack_gts fed from datapath.unpack_batch."""
import types

import numpy as np
import pytest
import torch

import ingest_ref as R


def test_plan_point_capacity_arithmetic():
    from uni3detr_amd.trainer import plan_point_capacity as plan
    assert plan([1000]) == 2048                                   # 1250 -> next multiple of 1024
    assert plan([1000, 819]) == 2048
    assert plan([820], margin=1.25, multiple=1024) == 2048       # 1025 -> 2048
    assert plan([819], margin=1.25, multiple=1024) == 1024       # ceil(1023.75) = 1024
    assert plan([[250000, 281234], [263000, 20]]) == 352256      # ceil(351542.5) = 351543 -> 344 * 1024
    assert plan([100], margin=1.0, multiple=1) == 100
    assert plan([0]) == 1024                                      # at least one multiple
    assert plan([4096], margin=1.0) == 4096
    assert plan([4097], margin=1.0) == 5120
    assert plan(np.array([7, 9]), margin=1.5, multiple=8) == 16   # ceil(13.5) = 14 -> 16
    for bad in ([], [[-1]]):
        with pytest.raises(ValueError):
            plan(bad)
    with pytest.raises(ValueError):
        plan([10], margin=0.9)


def test_capacity_mode_refuses_what_it_does_not_serve():
    """Decided before anything touches the device: dynamic voxelization, the torch.optim update, a capacity below the initial batch,
    set_packed_batch on a fixed-layout step or on a batch whose sweeps were not merged."""
    from uni3detr_amd.trainer import TrainStep
    pts = [torch.zeros((40, 4)), torch.zeros((70, 4))]
    with pytest.raises(NotImplementedError, match="dynamic_voxelization"):
        TrainStep(types.SimpleNamespace(dynamic_voxelization=True), pts, [], [], point_capacity=1024)
    with pytest.raises(NotImplementedError, match="flat_update"):
        TrainStep(types.SimpleNamespace(dynamic_voxelization=False), pts, [], [], point_capacity=1024, flat_update=False)
    with pytest.raises(ValueError, match="point_capacity 64"):
        TrainStep(types.SimpleNamespace(dynamic_voxelization=False), pts, [], [], point_capacity=64)
    with pytest.raises(RuntimeError, match="point_capacity"):
        TrainStep.set_packed_batch(types.SimpleNamespace(point_capacity=None), dict(points=pts[0]))
    with pytest.raises(ValueError, match="sweeps"):
        TrainStep.set_packed_batch(types.SimpleNamespace(point_capacity=64), dict(points=pts[0], sweeps={}))


def _pts(n, F):
    return (np.arange(n * F, dtype=np.float32).reshape(n, F) + 1) * np.float32(0.5)


def test_ingest_ref_points_count_empty_scene_and_overflow():
    F, P = 4, 3
    pts = _pts(12, F)
    off = np.array([0, 4, 4, 9, 12], np.int32)                    # scene 1 is empty
    cnt = np.array([2, 0, 5, 3], np.int32)                        # scene 0: count shorter than its segment; scene 2: 5 live > P
    cat = np.full((4 * P + 2, F), -7.0, np.float32)
    out = R.batch_ingest(pts, off, cnt, P, cat)
    assert out["dst_off"].tolist() == [0, 2, 2, 5, 8]
    assert np.array_equal(cat[:2], pts[0:2]) and np.array_equal(cat[2:5], pts[4:7]) and np.array_equal(cat[5:8], pts[9:12])
    assert (cat[8:] == -7.0).all()                                # nothing behind the live rows, nothing behind B * P
    assert out["flag"] == 1.0 and out["overflow"].tolist() == [1, 0]
    # without count: whole segments; nothing over P = 5; the flag is added to
    cat = np.full((4 * 5, F), -7.0, np.float32)
    out = R.batch_ingest(pts, off, None, 5, cat, flag=2.0)
    assert out["dst_off"].tolist() == [0, 4, 4, 9, 12] and np.array_equal(cat[:12], pts)
    assert out["flag"] == 2.0 and out["overflow"].tolist() == [0, 0]
    # a count above its segment is clamped to the segment, a negative one to zero
    cat = np.full((4 * 5, F), -7.0, np.float32)
    out = R.batch_ingest(pts, off, np.array([9, 3, -2, 1], np.int32), 5, cat)
    assert out["dst_off"].tolist() == [0, 4, 4, 4, 5] and np.array_equal(cat[4], pts[9])


def test_ingest_ref_boxes_padding_gravity_centre_and_overflow():
    gt7 = np.array([[1, 2, 3, 4, 5, 6, 0.5], [10, 20, -1.5, 2, 2, 3, -1.0], [0, 0, 0, 1, 1, 1, 0]], np.float32)
    lab = np.array([4, 2, 9], np.int32)
    goff = np.array([0, 2, 3], np.int32)
    pts, off = _pts(2, 4), np.array([0, 1, 2], np.int32)
    cat = np.zeros((4, 4), np.float32)
    # 7 -> 9 columns: zero velocities; z -> z + dz / 2
    out9, l9 = np.full((2 * 2 + 1, 9), -7.0, np.float32), np.full(2 * 2 + 1, -7, np.int32)
    r = R.batch_ingest(pts, off, None, 2, cat, gt7, lab, goff, None, 2, out9, l9)
    assert r["gt_off"].tolist() == [0, 2, 3] and r["flag"] == 0.0
    assert out9[0].tolist() == [1, 2, 6, 4, 5, 6, 0.5, 0, 0] and out9[1].tolist() == [10, 20, 0, 2, 2, 3, -1.0, 0, 0]
    assert out9[2].tolist() == [0, 0, 0.5, 1, 1, 1, 0, 0, 0] and (out9[3:] == -7.0).all()
    assert l9.tolist() == [4, 2, 9, -7, -7]
    # 9 columns kept; gt_count shorter than the segment; boxes over G = 1 are cut and flagged
    gt9 = np.concatenate([gt7, np.array([[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]], np.float32)], 1)
    out, lo = np.full((2, 9), -7.0, np.float32), np.full(2, -7, np.int32)
    r = R.batch_ingest(pts, off, None, 2, cat, gt9, lab, goff, None, 1, out, lo)
    assert r["gt_off"].tolist() == [0, 1, 2] and r["flag"] == 1.0 and r["overflow"].tolist() == [0, 1]
    assert out[0].tolist() == [1, 2, 6, 4, 5, 6, 0.5, np.float32(0.1), np.float32(0.2)] and out[1, 0] == 0 and lo.tolist() == [4, 9]
    out, lo = np.full((4, 7), -7.0, np.float32), np.full(4, -7, np.int32)
    r = R.batch_ingest(pts, off, None, 2, cat, gt9, lab, goff, np.array([1, 0], np.int32), 2, out, lo)       # 9 -> 7 columns: cut
    assert r["gt_off"].tolist() == [0, 1, 1] and out[0].tolist() == [1, 2, 6, 4, 5, 6, 0.5] and (out[1:] == -7.0).all()
    # no boxes at all: offsets of zeros
    r = R.batch_ingest(pts, off, None, 2, cat, None, None, None, None, 2, out, lo)
    assert r["gt_off"].tolist() == [0, 0, 0]


@pytest.mark.parametrize("dim,gd", [(7, 7), (7, 9), (9, 9), (9, 7)])
def test_ingest_ref_boxes_equal_pack_gts_from_unpack_batch(dim, gd):
    """The GT half of the ingest is Uni3DETRHead._pack_gts applied to what unpack_batch hands the trainer, bit for bit."""
    from uni3detr_amd import datapath as dp
    from uni3detr_amd.plugin.head import Uni3DETRHead
    rng = np.random.default_rng(dim * 10 + gd)
    for trial in range(6):
        B = int(rng.integers(1, 6))
        sizes = [int(v) for v in rng.integers(0, 9, B)]
        if trial == 0:
            sizes[0] = 0
        boxes = [torch.from_numpy(rng.normal(0, 10, (g, dim)).astype(np.float32)) for g in sizes]
        labels = [torch.from_numpy(rng.integers(0, 10, g).astype(np.int32)) for g in sizes]
        batch = dp.pack_batch([torch.zeros((3, 4))] * B, boxes, "LiDAR", gt_labels_3d=labels)
        if trial % 2:
            batch["gt_count"] = torch.tensor([int(rng.integers(0, g + 1)) for g in sizes], dtype=torch.int32)
        _, gts, labs = dp.unpack_batch(batch)
        want_gt, want_lab, want_off, gmax = Uni3DETRHead._pack_gts(types.SimpleNamespace(gt_dim=gd), gts, labs, torch.device("cpu"))
        G = max(gmax, 1)
        out, lo = np.full((B * G, gd), -7.0, np.float32), np.full(B * G, -7, np.int32)
        cnt = batch["gt_count"].numpy() if "gt_count" in batch else None
        r = R.batch_ingest(np.zeros((3 * B, 4), np.float32), batch["scene_off"].numpy(), None, 3, np.zeros((3 * B, 4), np.float32),
                           batch["gt_bboxes_3d"].numpy(), batch["gt_labels_3d"].numpy(), batch["gt_off"].numpy(), cnt, G, out, lo)
        n = int(want_off[-1])
        assert r["gt_off"].tolist() == want_off.tolist() and r["flag"] == 0.0
        assert np.array_equal(out[:n], want_gt.numpy()) and np.array_equal(lo[:n], want_lab.numpy())
        assert (out[n:] == -7.0).all()
