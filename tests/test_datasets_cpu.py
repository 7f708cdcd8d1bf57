"""datasets.samples_from_cfg on synthetic info pickles of the four dataset kinds (3 to 4 samples each, one without boxes): the sample
dicts in the feeder's shape, filter_empty_gt, KITTI's DontCare rows, the nuScenes valid flag and load_interval, the RepeatDataset /
CBGSDataset unwrapping, and the restricted unpickler."""
import pickle

import numpy as np
import pytest

from uni3detr_amd import datasets as D
from uni3detr_amd.training import EpochPlan


def _dump(path, obj):
    with open(path, "wb") as f:
        pickle.dump(obj, f)
    return str(path)


def _check_shape(samples, dim):
    for s in samples:
        assert set(s) == {"pts_filename", "gt_bboxes_3d", "gt_labels_3d", "info"} and isinstance(s["pts_filename"], str)
        g, l = s["gt_bboxes_3d"], s["gt_labels_3d"]
        assert g.dtype == np.float32 and g.ndim == 2 and g.shape[1] == dim and l.dtype == np.int64 and l.shape == (g.shape[0],)


# ---- indoor -------------------------------------------------------------------------------------------------------------------------
def _indoor_infos(cols):
    rng = np.random.RandomState(0)
    infos = []
    for k, n in enumerate((2, 0, 3)):
        annos = dict(gt_num=n)
        if n:
            annos.update(gt_boxes_upright_depth=rng.uniform(0.5, 2.0, (n, cols)), name=np.array(["chair", "bed", "desk"][:n]),
                         **{"class": np.array([3, 1, 5][:n])})
        infos.append(dict(point_cloud=dict(num_features=6, lidar_idx=k), pts_path=f"points/{k:06d}.bin", annos=annos))
    return infos


@pytest.mark.parametrize("kind, cols", [("SUNRGBDDataset", 7), ("ScanNetDataset", 6)])
def test_indoor(tmp_path, kind, cols):
    infos = _indoor_infos(cols)
    ann = _dump(tmp_path / "infos.pkl", infos)
    base = dict(type=kind, data_root=str(tmp_path), ann_file=ann, pipeline=[dict(type="LoadPointsFromFile")], box_type_3d="Depth")
    samples, meta = D.samples_from_cfg(dict(type="RepeatDataset", times=5, dataset=dict(base, filter_empty_gt=False)))
    assert len(samples) == 3 and meta["repeat"] == 5 and meta["class_ids"] is None and meta["kind"] == "indoor"
    assert meta["box_type_3d"] == "Depth" and len(meta["classes"]) == (10 if cols == 7 else 18)
    _check_shape(samples, 7)
    assert samples[0]["pts_filename"] == str(tmp_path / "points" / "000000.bin") and samples[1]["gt_bboxes_3d"].shape == (0, 7)
    raw = infos[0]["annos"]["gt_boxes_upright_depth"].astype(np.float32)
    got = samples[0]["gt_bboxes_3d"]
    assert np.array_equal(got[:, [0, 1, 3, 4, 5]], raw[:, [0, 1, 3, 4, 5]])
    assert np.array_equal(got[:, 2], raw[:, 2] + raw[:, 5] * np.float32(-0.5))      # gravity centre -> bottom centre
    assert np.array_equal(got[:, 6], raw[:, 6] if cols == 7 else np.zeros(2, np.float32))
    assert samples[2]["gt_labels_3d"].tolist() == [3, 1, 5]
    # the evaluator's ground truth: gravity-centre rows and labels per sample
    assert np.array_equal(meta["gt_boxes"][0][:, :cols], raw) and meta["gt_labels"][2].tolist() == [3, 1, 5] and len(meta["infos"]) == 3
    # filter_empty_gt (the default) drops the empty sample from a training set, never from a test set
    samples, meta = D.samples_from_cfg(base)
    assert [s["pts_filename"][-10:] for s in samples] == ["000000.bin", "000002.bin"] and meta["repeat"] == 1 and len(meta["gt_boxes"]) == 2
    samples, meta = D.samples_from_cfg(dict(base, test_mode=True))
    assert len(samples) == 3 and meta["test_mode"]
    # a `classes` subset numbers the labels by name
    samples, _ = D.samples_from_cfg(dict(base, classes=["bed", "chair"]))
    assert samples[0]["gt_labels_3d"].tolist() == [1, 0] and samples[1]["gt_labels_3d"].tolist() == [1, 0, -1]


# ---- KITTI --------------------------------------------------------------------------------------------------------------------------
def _kitti_infos():
    rng = np.random.RandomState(1)
    eye = np.eye(4)
    out = []
    for k, names in enumerate((["Car", "DontCare", "Pedestrian"], ["DontCare"], ["Van", "Cyclist"], [])):
        n = len(names)
        annos = dict(name=np.array(names, dtype="<U10"), location=rng.uniform(1, 20, (n, 3)), dimensions=rng.uniform(1, 4, (n, 3)),
                     rotation_y=rng.uniform(-3, 3, n), difficulty=np.zeros(n, np.int32))
        out.append(dict(image=dict(image_idx=k, image_shape=np.array([375, 1242])), point_cloud=dict(velodyne_path=f"training/velodyne/{k:06d}.bin"),
                        calib=dict(R0_rect=eye, Tr_velo_to_cam=eye, P2=eye), annos=annos))
    return out


def test_kitti(tmp_path):
    ann = _dump(tmp_path / "kitti_infos_train.pkl", _kitti_infos())
    classes = ["Pedestrian", "Cyclist", "Car"]
    base = dict(type="KittiDataset", data_root=str(tmp_path), ann_file=ann, split="training", pts_prefix="velodyne_reduced", classes=classes,
                box_type_3d="LiDAR")
    samples, meta = D.samples_from_cfg(dict(type="RepeatDataset", times=2, dataset=base))
    _check_shape(samples, 7)
    assert meta["repeat"] == 2 and meta["kind"] == "kitti" and meta["box_type_3d"] == "LiDAR"
    # samples 1 (DontCare only) and 3 (no object) have no box of a known class: filtered; DontCare rows are dropped, Van stays as -1
    assert [s["pts_filename"] for s in samples] == [str(tmp_path / "training" / "velodyne_reduced" / f"{k:06d}.bin") for k in (0, 2)]
    assert samples[0]["gt_labels_3d"].tolist() == [2, 0] and samples[1]["gt_labels_3d"].tolist() == [-1, 1]
    assert [int(i["image"]["image_idx"]) for i in meta["infos"]] == [0, 2]
    samples, _ = D.samples_from_cfg(dict(base, filter_empty_gt=False, split=None))
    assert len(samples) == 4 and samples[1]["gt_bboxes_3d"].shape == (0, 7) and samples[3]["gt_bboxes_3d"].shape == (0, 7)
    assert samples[0]["pts_filename"] == str(tmp_path / "training" / "velodyne" / "000000.bin")


# ---- nuScenes -----------------------------------------------------------------------------------------------------------------------
NUSC = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone"]


def _nusc_infos():
    rng = np.random.RandomState(2)
    rows = ((["car", "pedestrian"], [True, True]), ([], []), (["truck", "car"], [False, True]), (["bus"], [False]))
    infos = []
    for k, (names, valid) in enumerate(rows):
        n = len(names)
        vel = rng.uniform(-1, 1, (n, 2))
        if n:
            vel[0] = np.nan
        infos.append(dict(token=f"tok{k}", lidar_path=f"samples/LIDAR_TOP/{k}.bin", timestamp=1_000_000 * (10 - k),
                          sweeps=[dict(data_path=f"sweeps/LIDAR_TOP/{k}_{j}.bin", timestamp=1_000_000 * (10 - k) - 50_000 * (j + 1),
                                       sensor2lidar_rotation=np.eye(3), sensor2lidar_translation=np.zeros(3)) for j in range(2)],
                          gt_boxes=rng.uniform(1, 5, (n, 7)), gt_names=np.array(names, dtype="<U24"), gt_velocity=vel,
                          valid_flag=np.array(valid, bool), num_lidar_pts=np.array([5] * n)))
    return dict(infos=infos, metadata=dict(version="v1.0-mini"))


def test_nuscenes(tmp_path):
    ann = _dump(tmp_path / "nuscenes_infos_train.pkl", _nusc_infos())
    base = dict(type="NuScenesSweepDataset", data_root=str(tmp_path), ann_file=ann, classes=NUSC, use_valid_flag=True, box_type_3d="LiDAR")
    samples, meta = D.samples_from_cfg(dict(type="CBGSDataset", dataset=base))
    _check_shape(samples, 9)
    # sorted by timestamp (the file's order reversed); sample 1 has no box, sample 3 no VALID box: both filtered
    assert [s["pts_filename"] for s in samples] == [str(tmp_path / "samples" / "LIDAR_TOP" / f"{k}.bin") for k in (2, 0)]
    assert samples[0]["gt_labels_3d"].tolist() == [0] and samples[1]["gt_labels_3d"].tolist() == [0, 8]       # the invalid truck is gone
    assert meta["class_ids"] == [[0], [0, 8]] and meta["repeat"] == 1 and [i["token"] for i in meta["infos"]] == ["tok2", "tok0"]
    assert samples[1]["gt_bboxes_3d"][0, 7:].tolist() == [0.0, 0.0]                                            # NaN velocity -> 0
    info = samples[0]["info"]
    assert info["timestamp"] == 8.0 and [s["data_path"] for s in info["sweeps"]] == [str(tmp_path / "sweeps" / "LIDAR_TOP" / f"2_{j}.bin")
                                                                                    for j in range(2)]
    plan = EpochPlan(len(samples), 1, class_ids=meta["class_ids"])
    assert len(plan) == 2                                      # class 0: int(2 * .5 / (2 / 3)) = 1 draw, class 8: int(1 * .5 / (1 / 3)) = 1
    # without the valid flag the boxes with lidar points count; load_interval thins the time-sorted list
    samples, meta = D.samples_from_cfg(dict(base, use_valid_flag=False, filter_empty_gt=False, load_interval=2, with_velocity=False))
    assert [i["token"] for i in meta["infos"]] == ["tok3", "tok1"] and samples[0]["gt_labels_3d"].tolist() == [3]
    assert samples[0]["gt_bboxes_3d"].shape == (1, 7) and samples[1]["gt_bboxes_3d"].shape == (0, 7) and meta["class_ids"] is None


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
class _Thing:
    def __init__(self):
        self.x = 1


def test_object_pickles_need_trusted(tmp_path):
    infos = _indoor_infos(7)
    infos[0]["extra"] = _Thing()
    ann = _dump(tmp_path / "objects.pkl", infos)
    cfg = dict(type="SUNRGBDDataset", data_root=str(tmp_path), ann_file=ann)
    with pytest.raises(RuntimeError, match="trusted"):
        D.samples_from_cfg(cfg)
    samples, _ = D.samples_from_cfg(cfg, trusted=True)
    assert len(samples) == 2


def test_unknown_dataset_type(tmp_path):
    with pytest.raises(NotImplementedError, match="WaymoDataset"):
        D.samples_from_cfg(dict(type="RepeatDataset", times=2, dataset=dict(type="WaymoDataset", ann_file="x")))
