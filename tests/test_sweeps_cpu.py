"""Host side of the on-device LiDAR sweep merge, PointShuffle and ObjectNameFilter: read_sweeps (choice draw, file reads, replay)
against the loop-by-loop restatement (tests/sweeps_ref.py), the opt-ins and errors of DevicePipeline, and the float64 formula of the
device transform against upstream's `@` form."""
import copy

import numpy as np
import pytest
import torch

import sweeps_ref as R

ENTRY = dict(type="LoadPointsFromMultiSweeps", sweeps_num=9, use_dim=[0, 1, 2, 3, 4], pad_empty_sweeps=True, remove_close=True)


def _rot(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def write_sweeps(tmp_path, rng, sizes, load_dim=5, prefix="s"):
    """one .bin per entry of sizes (float32 rows of load_dim columns, a few rows near the origin) -> the info's sweep dicts."""
    out = []
    for j, n in enumerate(sizes):
        a = rng.uniform(-30, 30, (n, load_dim)).astype(np.float32)
        a[: n // 8, :2] = rng.uniform(-1.2, 1.2, (n // 8, 2)).astype(np.float32)
        path = str(tmp_path / f"{prefix}{j}.bin")
        a.tofile(path)
        out.append(dict(data_path=path, timestamp=1_533_151_603_000_000 - 50_000 * (j + 1), sensor2lidar_rotation=_rot(rng),
                        sensor2lidar_translation=rng.normal(size=3) * 0.5))
    return out


def _info(sweeps):
    return dict(timestamp=1_533_151_603_547_000 / 1e6, sweeps=sweeps)


@pytest.mark.parametrize("n_sweeps,test_mode", [(4, False), (9, False), (15, True), (15, False), (0, False)])
def test_read_sweeps_matches_restatement(tmp_path, n_sweeps, test_mode):
    from uni3detr_amd import datapath as dp
    rng = np.random.default_rng(n_sweeps + 10 * test_mode)
    sweeps = write_sweeps(tmp_path, rng, [int(v) for v in rng.integers(0, 700, n_sweeps)])
    entry = dict(ENTRY, test_mode=test_mode)
    np.random.seed(3)
    rec = dp.read_sweeps(_info(sweeps), entry)
    np.random.seed(3)
    key = rng.uniform(-20, 20, (300, 5)).astype(np.float32)
    ref, ref_choices = R.load_points_from_multi_sweeps(key, sweeps, _info(sweeps)["timestamp"], 9, 5, [0, 1, 2, 3, 4], True, True,
                                                       test_mode)
    assert np.array_equal(rec["choices"], ref_choices)
    if n_sweeps > 9 and not test_mode:
        assert not np.array_equal(rec["choices"], np.arange(9))           # a draw, not the first nine
    assert rec["pad"] == (n_sweeps == 0) and rec["sweeps_num"] == 9 and rec["load_dim"] == 5
    assert len(rec["points"]) == len(ref_choices) == rec["rot"].shape[0] == rec["trans"].shape[0] == rec["dt"].shape[0]
    for j, idx in enumerate(ref_choices):
        sw = sweeps[idx]
        assert np.array_equal(rec["points"][j], np.fromfile(sw["data_path"], np.float32).reshape(-1, 5))
        assert np.array_equal(rec["rot"][j], sw["sensor2lidar_rotation"]) and np.array_equal(rec["trans"][j], sw["sensor2lidar_translation"])
        assert rec["dt"][j] == _info(sweeps)["timestamp"] - sw["timestamp"] / 1e6
    # the restated merge assembled from the record equals the restatement reading the files itself
    parts = [np.concatenate([key[:, :4], np.zeros((len(key), 1), np.float32)], 1)]
    if rec["pad"]:
        parts += [R.remove_close(parts[0])] * 9
    for j in range(len(rec["points"])):
        p = R.remove_close(rec["points"][j].copy())
        p[:, :3] = R.rotate_translate(p[:, :3], rec["rot"][j], rec["trans"][j])
        p[:, 4] = rec["dt"][j]
        parts.append(p)
    assert np.array_equal(np.concatenate(parts), ref)


def test_read_sweeps_without_padding_and_replay(tmp_path):
    from uni3detr_amd import datapath as dp
    rng = np.random.default_rng(7)
    rec = dp.read_sweeps(_info([]), dict(ENTRY, pad_empty_sweeps=False))
    assert not rec["pad"] and rec["points"] == [] and rec["choices"].shape == (0,)
    sweeps = write_sweeps(tmp_path, rng, [50] * 12)
    np.random.seed(11)
    first = dp.read_sweeps(_info(sweeps), ENTRY)
    state = np.random.get_state()
    again = dp.read_sweeps(_info(sweeps), ENTRY, choices=first["choices"])      # a recorded batch["sweep_choices"][b]
    assert np.array_equal(again["choices"], first["choices"])
    assert all(np.array_equal(a, b) for a, b in zip(again["points"], first["points"]))
    assert np.array_equal(np.random.get_state()[1], state[1])                   # the replay draws nothing
    own = dp.read_sweeps(_info(sweeps), ENTRY, rng=np.random.RandomState(11))
    assert np.array_equal(own["choices"], first["choices"])                     # an explicit generator, same stream


def _ordered(a):
    """float32 -> int64 on one line: adjacent floats differ by 1 (across zero too)."""
    i = a.view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def test_explicit_order_is_within_one_ulp_of_the_matmul_form():
    rng = np.random.default_rng(5)
    worst = 0
    for k in range(20):
        xyz = (rng.uniform(-60, 60, (20000, 3)) * (10.0 ** rng.uniform(-3, 0, (20000, 1)))).astype(np.float32)
        rot, trans = _rot(rng), rng.normal(size=3) * 2
        a = R.rotate_translate(xyz, rot, trans)
        b = R.rotate_translate(xyz, rot, trans, explicit=True)
        worst = max(worst, int(np.abs(_ordered(a) - _ordered(b)).max()))
    assert worst <= 1


def test_object_name_filter_restatement():
    boxes = np.arange(6 * 7, dtype=np.float32).reshape(6, 7)
    labels = np.array([0, -1, 2, 3, 1, -1])
    b, l = R.object_name_filter(boxes, labels, ["car", "truck", "bus"])
    assert np.array_equal(l, [0, 2, 1]) and np.array_equal(b, boxes[[0, 2, 4]])


def test_device_pipeline_opt_ins_and_errors():
    from uni3detr_amd import datapath as dp
    from uni3detr_amd.configs import pipelines as P
    for name in ("kitti_3classes", "kitti_car", "nuscenes"):
        cfg = P.SHIPPED[name]["train_pipeline"]
        pipe = dp.DevicePipeline(cfg)
        assert "ObjectNameFilter" in pipe.skipped and "PointShuffle" in pipe.skipped
        assert ("LoadPointsFromMultiSweeps" in pipe.skipped) == (name == "nuscenes")
        named = copy.deepcopy(cfg)
        for c in named:
            if c["type"] == "ObjectNameFilter":
                c["classes"] = ["a", "b", "c"]
        pipe = dp.DevicePipeline(named, sweeps=True, point_shuffle=True, name_filter=True)
        names = [type(t).__name__ for t in pipe.transforms]
        assert not {"ObjectNameFilter", "PointShuffle", "LoadPointsFromMultiSweeps"} & set(pipe.skipped)
        assert "ObjectNameFilter" in names and "PointShuffle" in names
        assert names.index("ObjectNameFilter") == names.index("ObjectRangeFilter") + 1
        assert names.index("PointShuffle") == names.index("ObjectNameFilter") + 1
        assert ("LoadPointsFromMultiSweeps" in names) == (name == "nuscenes")
    test = dp.DevicePipeline(P.SHIPPED["nuscenes"]["test_pipeline"], sweeps=True)
    assert [type(t).__name__ for t in test.transforms] == ["LoadPointsFromMultiSweeps", "PointsRangeFilter"]
    # one flag at a time
    pipe = dp.DevicePipeline(P.SHIPPED["nuscenes"]["train_pipeline"], point_shuffle=True)
    assert "LoadPointsFromMultiSweeps" in pipe.skipped and "ObjectNameFilter" in pipe.skipped and "PointShuffle" not in pipe.skipped
    # upstream's constructor arguments
    m = dp.OBJECT_AUG.build(ENTRY)
    assert (m.sweeps_num, m.load_dim, m.use_dim, m.pad_empty_sweeps, m.remove_close, m.test_mode) == (9, 5, [0, 1, 2, 3, 4], True, True,
                                                                                                      False)
    d = dp.OBJECT_AUG.build(dict(type="LoadPointsFromMultiSweeps"))
    assert (d.sweeps_num, d.load_dim, d.use_dim, d.pad_empty_sweeps, d.remove_close) == (10, 5, [0, 1, 2, 4], False, False)
    dp.OBJECT_AUG.build(dict(ENTRY, file_client_args=dict(backend="disk")))
    with pytest.raises(NotImplementedError):
        dp.OBJECT_AUG.build(dict(ENTRY, file_client_args=dict(backend="petrel")))
    with pytest.raises(NotImplementedError):
        dp.OBJECT_AUG.build(dict(ENTRY, remove_close=2.0))
    with pytest.raises(NotImplementedError):
        dp.read_sweeps(_info([]), dict(ENTRY, file_client_args=dict(backend="petrel")))
    with pytest.raises(TypeError):
        dp.OBJECT_AUG.build(dict(type="ObjectNameFilter"))                   # upstream: classes is required
    # sweeps=True on a batch without batch["sweeps"]
    merge = dp.DevicePipeline([ENTRY], sweeps=True)
    with pytest.raises(KeyError):
        merge(dict(points=torch.zeros((4, 5)), scene_off=torch.tensor([0, 4], dtype=torch.int32)))


def test_replicate_takes_spare_rows_past_the_last_scene():
    """MultiScaleFlipAug3D's gather on a batch with spare rows past scene_off[-1] (what the sweep merge leaves): every view of every
    scene is exact, the repeat counts add up to the output size, the spare rows stay past the new last offset."""
    from uni3detr_amd import datapath as dp
    x = torch.arange(20, dtype=torch.float32).reshape(10, 2)
    off = torch.tensor([0, 3, 3, 7], dtype=torch.int32)                   # rows 7..9 are spare
    rows, off_v = dp._replicate(x, off, 2)
    assert rows.shape == (20, 2) and off_v.tolist() == [0, 3, 6, 6, 6, 10, 14]
    for s, (a, b) in enumerate([(0, 3), (0, 3), (3, 3), (3, 3), (3, 7), (3, 7)]):
        assert torch.equal(rows[off_v[s]:off_v[s + 1]], x[a:b])
    assert torch.equal(rows[14:], x[[7, 8, 9, 9, 9, 9]])                 # spare rows: x's spare rows, then its last row; never out of range
    # an exactly packed input expands as before
    rows, off_v = dp._replicate(x[:7], off, 3)
    assert rows.shape == (21, 2) and off_v.tolist() == [0, 3, 6, 9, 9, 9, 9, 13, 17, 21]
    assert torch.equal(rows[9:13], x[3:7]) and torch.equal(rows[17:21], x[3:7])


def test_sweep_upload_refuses_int32_overflow_of_the_merged_rows():
    """nine pad copies of a 2^28-row key frame: no raw sweep row, but 10 * 2^28 merged rows do not fit the device's int32 offsets."""
    from uni3detr_amd import datapath as dp
    rec = dict(points=[], rot=np.zeros((0, 3, 3)), trans=np.zeros((0, 3)), dt=np.zeros(0), choices=np.zeros(0, np.int64), pad=True,
               sweeps_num=9, load_dim=5)
    with pytest.raises(ValueError, match="2\\^31"):
        dp._upload_sweeps([rec], [2 ** 28], 5, torch.device("cpu"))
