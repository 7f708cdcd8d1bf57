"""Host side of the on-device GT-paste database builder (uni3detr_amd/gtdb.py): the loop restatement (tests/gtdb_ref.py) on hand-made
scenes, the info bookkeeping against it, the schema, the pickle / .bin and packed writers round-tripping through from_infos and
from_packed on the CPU, the command line and the info adapters, and the entry points being part of the build."""
import os
import pickle

import numpy as np
import pytest
import torch

import gtdb_ref as R

BOX = [0.0, 0.0, 0.0, 2.0, 2.0, 2.0, 0.0]


def _scenes():
    """two scenes: A holds overlapping boxes 0/1, an empty box 2 and a `Van` 3; B gives group ids, difficulty, a valid flag and scores"""
    a_boxes = np.array([BOX, [0.5, 0, 0, 2, 2, 2, 0], [30, 30, 0, 1, 1, 1, 0.3], [-10, 0, 0, 2, 4, 2, np.pi / 2]], np.float32)
    a_pts = np.array([[0.2, 0.1, 0.5, 7], [-0.8, 0, 0.5, 8], [1.2, 0, 1.0, 9], [9, 9, 9, 1], [0.6, -0.5, 1.5, 2], [-11.5, 0.3, 1, 3],
                      [-10, 1.5, 1, 4]], np.float32)
    b_boxes = np.array([[5, 5, -1, 2, 2, 2, 0.2], [5.2, 5, -1, 2, 2, 2, 0.1], [-5, -5, -1, 2, 2, 2, 0], [0, 8, -1, 3, 3, 3, 1.0]], np.float32)
    rng = np.random.default_rng(0)
    b_pts = np.concatenate([rng.uniform(-0.8, 0.8, (40, 4)) + [5, 5, 0, 0], rng.uniform(-0.8, 0.8, (20, 4)) + [-5, -5, 0, 0],
                            rng.uniform(-1, 1, (10, 4)) + [0, 8, 0.5, 0]]).astype(np.float32)
    return [dict(sample_idx=7, points=a_pts, gt_bboxes_3d=a_boxes, gt_names=np.array(["Car", "Pedestrian", "Car", "Van"])),
            dict(sample_idx="tok", points=b_pts, gt_bboxes_3d=b_boxes, gt_names=np.array(["Pedestrian", "Car", "Car", "Cyclist"]),
                 group_ids=np.array([4, 4, 9, 4]), difficulty=np.array([2, 0, 1, -1], np.int32),
                 valid_flag=np.array([True, True, False, True]), score=np.array([0.5, 0.25, 0.75, 1.0], np.float32))]


def test_restatement_hand_made():
    infos, objs = R.create_groundtruth_database(_scenes(), "kitti")
    assert list(infos) == ["Car", "Pedestrian", "Van", "Cyclist"]                       # first appearance
    car0, ped0 = objs["Car"][0], objs["Pedestrian"][0]
    # a point in two boxes lands in both, scene order kept, relative to each box's bottom centre, the other columns untouched
    assert np.array_equal(car0, np.array([[0.2, 0.1, 0.5, 7], [-0.8, 0, 0.5, 8], [0.6, -0.5, 1.5, 2]], np.float32))
    assert np.array_equal(ped0, np.array([[0.2, 0.1, 0.5, 7], [1.2, 0, 1.0, 9], [0.6, -0.5, 1.5, 2]], np.float32) - np.float32([0.5, 0, 0, 0]))
    assert objs["Car"][1].shape == (0, 4) and infos["Car"][1]["num_points_in_gt"] == 0   # an empty object stays, with no points
    assert [i["gt_idx"] for i in infos["Car"]] == [0, 2, 1] and infos["Van"][0]["gt_idx"] == 3
    # the box turned by pi / 2: dy = 4 lies along x, so (-11.5, 0.3) is inside and (-10, 1.5) is not
    assert np.array_equal(objs["Van"][0], np.array([[-1.5, 0.3, 1, 3]], np.float32))
    # without group_ids every box is its own group; scene B: groups 4, 4, 4 (box 2 is dropped by the valid flag, it takes no gt_idx)
    assert [i["group_id"] for k in ("Car", "Pedestrian", "Van") for i in infos[k] if i["image_idx"] == 7] == [0, 2, 1, 3]
    b = [i for k in infos for i in infos[k] if i["image_idx"] == "tok"]
    assert sorted((i["gt_idx"], i["group_id"]) for i in b) == [(0, 4), (1, 4), (2, 4)]
    assert infos["Cyclist"][0]["gt_idx"] == 2 and infos["Cyclist"][0]["difficulty"] == -1 and infos["Cyclist"][0]["score"] == 1.0
    assert infos["Car"][0]["difficulty"] == 0 and "score" not in infos["Car"][0]
    assert infos["Car"][0]["path"] == os.path.join("kitti_gt_database", "pts_dir", "7_Car_0.bin")


def test_used_classes_keep_gt_idx_and_group_counter():
    infos, _ = R.create_groundtruth_database(_scenes(), "x", used_classes=["Car", "Cyclist"])
    assert list(infos) == ["Car", "Cyclist"]
    assert [(i["image_idx"], i["gt_idx"], i["group_id"]) for i in infos["Car"]] == [(7, 0, 0), (7, 2, 1), ("tok", 1, 2)]
    assert [(i["gt_idx"], i["group_id"]) for i in infos["Cyclist"]] == [(2, 2)]          # group 4 again: the same id as the Car


def _builder_infos(scenes, prefix, used=None):
    """DbInfoBuilder fed with the restatement's counts -> (db_infos, scene-major objects)"""
    from uni3detr_amd.gtdb import DbInfoBuilder
    b = DbInfoBuilder(prefix, used)
    objs = []
    for s in scenes:
        m = b.select(s)
        crops = R.crop_scene(s["points"], m["boxes"])
        b.add(m, [len(crops[i]) for i in m["gt_idx"]])
        objs += [crops[i] for i in m["gt_idx"]]
    return b, objs


@pytest.mark.parametrize("used", [None, ["Car", "Cyclist"], ["Pedestrian"]])
def test_builder_matches_restatement(used):
    b, objs = _builder_infos(_scenes(), "nusc", used)
    ref, ref_objs = R.create_groundtruth_database(_scenes(), "nusc", used)
    assert list(b.db_infos) == list(ref)
    for k in ref:
        assert len(b.db_infos[k]) == len(ref[k])
        for got, want in zip(b.db_infos[k], ref[k]):
            assert set(got) == set(want)
            for f in want:
                assert np.array_equal(got[f], want[f]), (k, f)
    order = b.key_major()
    flat = [o for k in ref for o in ref_objs[k]]
    assert len(order) == len(flat) and all(np.array_equal(objs[d], o) for d, o in zip(order, flat))


def test_schema_keys_and_dtypes():
    b, _ = _builder_infos(_scenes(), "p")
    keys = {"name", "path", "image_idx", "image_path", "image_crop_key", "image_crop_depth", "gt_idx", "box3d_lidar", "num_points_in_gt",
            "difficulty", "group_id"}
    for k, v in b.db_infos.items():
        for i in v:
            assert set(i) - {"score"} == keys and i["name"] == k
            assert i["box3d_lidar"].dtype == np.float32 and i["box3d_lidar"].shape == (7,)
            assert type(i["gt_idx"]) is int and type(i["num_points_in_gt"]) is int and type(i["group_id"]) is int
            assert np.issubdtype(np.asarray(i["difficulty"]).dtype, np.integer)
            assert i["image_path"] == "" and i["image_crop_key"] == "" and i["image_crop_depth"] == 0
    nine = dict(_scenes()[0], gt_bboxes_3d=np.concatenate([_scenes()[0]["gt_bboxes_3d"], np.ones((4, 2), np.float32)], 1))
    b9, _ = _builder_infos([nine], "p")
    assert b9.db_infos["Car"][0]["box3d_lidar"].shape == (9,)
    with pytest.raises(ValueError):
        _builder_infos([dict(_scenes()[0], gt_bboxes_3d=np.zeros((4, 8), np.float32))], "p")


def _same_database(a, b):
    assert a.classes == b.classes and len(a) == len(b)
    for f in ("points", "obj_off", "boxes", "labels"):
        x, y = getattr(a, f).cpu(), getattr(b, f).cpu()
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), f
    assert np.array_equal(a.num_points_in_gt, b.num_points_in_gt) and np.array_equal(a.difficulty, b.difficulty)
    assert list(a.rows) == list(b.rows) and all(np.array_equal(a.rows[k], b.rows[k]) for k in a.rows)
    assert [(k, s._example_num) for k, s in a.samplers.items()] == [(k, s._example_num) for k, s in b.samplers.items()]


def test_writers_round_trip_cpu(tmp_path):
    from uni3detr_amd import gtdb as G
    classes = ["Pedestrian", "Cyclist", "Car"]
    b, objs = _builder_infos(_scenes(), "kitti")
    off = np.concatenate([[0], np.cumsum([len(o) for o in objs])])
    pts = np.concatenate(objs)
    G.write_object_points(str(tmp_path), [b.db_infos[k][i] for k, i in b.order], pts, off)
    pkl = G.write_dbinfos(b.db_infos, str(tmp_path), "kitti")
    assert pkl == str(tmp_path / "kitti_dbinfos_train.pkl")
    with open(pkl, "rb") as f:
        assert list(pickle.load(f)) == list(b.db_infos)
    first = b.db_infos["Car"][0]
    assert np.array_equal(np.fromfile(tmp_path / first["path"], np.float32).reshape(-1, 4), objs[0])
    kp, ko = G._gather_objects(torch.from_numpy(pts), off, b.key_major())
    ref_p, ref_o = R.key_major(*R.create_groundtruth_database(_scenes(), "kitti"), 4)
    assert np.array_equal(kp.numpy(), ref_p) and np.array_equal(ko.numpy(), ref_o)
    G.write_packed(str(tmp_path / "db.npz"), b.db_infos, classes, kp, ko)
    with np.load(tmp_path / "db.npz", allow_pickle=False) as z:                 # readable without any pickle
        assert set(z.files) == set(G.PACKED_FIELDS)
    loader = dict(load_dim=4, use_dim=4)
    for prepare in (None, dict(filter_by_difficulty=[-1], filter_by_min_points=dict(Car=1, Pedestrian=5))):
        a = G.GTDatabase.from_infos(pkl, str(tmp_path), classes, prepare, points_loader=loader, device="cpu")
        c = G.GTDatabase.from_packed(str(tmp_path / "db.npz"), classes, prepare, device="cpu")
        _same_database(a, c)
    assert len(c) < len(b.order) and c.labels.tolist().count(-1) == 1              # the filters bit; `Van` is outside `classes`
    d = G._database(classes, b.db_infos, kp, ko, "cpu")
    _same_database(d, G.GTDatabase.from_packed(str(tmp_path / "db.npz"), classes, device="cpu"))


def test_build_needs_the_gpu_no_host_fallback():
    from uni3detr_amd import gtdb as G
    from uni3detr_amd.native import U3DError
    with pytest.raises(U3DError):
        G.create_groundtruth_database(_scenes(), ["Car"], info_prefix="k", device="cpu")
    with pytest.raises(ValueError):
        G.create_groundtruth_database(_scenes(), ["Car"], info_prefix="k", write_points=True)


def test_cli_arguments():
    from uni3detr_amd import gtdb as G
    a = G.parse_args(["--infos", "i.pkl", "--data-root", "d", "--dataset", "nuscenes", "--extra-tag", "nus", "--used-classes", "car", "bus",
                      "--packed", "o.npz", "--write-points"])
    assert (a.infos, a.data_root, a.dataset, a.extra_tag, a.used_classes, a.packed, a.write_points, a.trusted, a.chunk_scenes) == \
        ("i.pkl", "d", "nuscenes", "nus", ["car", "bus"], "o.npz", True, False, 8)
    a = G.parse_args(["--infos", "i", "--data-root", "d", "--dataset", "kitti", "--extra-tag", "kitti"])
    assert a.used_classes is None and a.packed is None and not a.write_points and a.chunk_scenes == 32
    for bad in (["--infos", "i", "--data-root", "d", "--dataset", "waymo", "--extra-tag", "t"], ["--infos", "i", "--dataset", "kitti"],
                ["--infos", "i", "--data-root", "d", "--dataset", "kitti", "--extra-tag", "t", "--chunk-scenes", "0"]):
        with pytest.raises(SystemExit):
            G.parse_args(bad)


class _Evil:
    def __reduce__(self):
        return (os.getcwd, ())


def test_info_file_loader_is_restricted(tmp_path):
    from uni3detr_amd import gtdb as G
    good = dict(infos=[dict(token="a", gt_boxes=np.zeros((2, 7)), timestamp=5, gt_names=np.array(["car", "bus"]))], metadata=dict(version="v"))
    with open(tmp_path / "good.pkl", "wb") as f:
        pickle.dump(good, f)
    got = G.load_info_file(str(tmp_path / "good.pkl"))
    assert got["infos"][0]["token"] == "a" and got["infos"][0]["gt_names"].tolist() == ["car", "bus"]
    with open(tmp_path / "evil.pkl", "wb") as f:
        pickle.dump([_Evil()], f)
    with pytest.raises(RuntimeError, match="trusted"):
        G.load_info_file(str(tmp_path / "evil.pkl"))
    assert G.load_info_file(str(tmp_path / "evil.pkl"), trusted=True) == [os.getcwd()]


def test_kitti_adapter(tmp_path):
    from uni3detr_amd import gtdb as G
    from uni3detr_amd.synth import kitti_scenes
    infos, _ = kitti_scenes(4, seed=3)
    for s, info in enumerate(infos):
        n = len(info["annos"]["name"])
        info["annos"]["difficulty"] = np.arange(n, dtype=np.int32) % 3
        info["annos"]["group_ids"] = np.arange(n, dtype=np.int32)
        info["point_cloud"] = dict(num_features=4, velodyne_path=f"velodyne/{s:06d}.bin")
        a, keep = info["annos"], info["annos"]["name"] != "DontCare"
        sc = G.kitti_scene(info, str(tmp_path))
        assert sc["sample_idx"] == s and sc["points_path"] == str(tmp_path / "velodyne" / f"{s:06d}.bin")
        assert sc["gt_names"].tolist() == a["name"][keep].tolist() and "DontCare" not in sc["gt_names"]
        assert np.array_equal(sc["difficulty"], a["difficulty"][keep]) and np.array_equal(sc["group_ids"], a["group_ids"][keep])
        b = sc["gt_bboxes_3d"]
        assert b.dtype == np.float32 and b.shape == (keep.sum(), 7)
        T = np.linalg.inv(info["calib"]["R0_rect"] @ info["calib"]["Tr_velo_to_cam"])
        for j, i in enumerate(np.nonzero(keep)[0]):
            want = T @ np.append(a["location"][i], 1.0)
            l, h, w = a["dimensions"][i]
            assert np.allclose(b[j, :3], want[:3], atol=1e-5) and np.allclose(b[j, 3:6], [l, w, h], atol=1e-6)
            assert -np.pi <= b[j, 6] < np.pi + 1e-6 and np.isclose(np.cos(b[j, 6]), np.cos(-a["rotation_y"][i] - np.pi / 2), atol=1e-5)


def test_nuscenes_adapter_and_scene_stream(tmp_path):
    from test_sweeps_cpu import write_sweeps
    from uni3detr_amd import gtdb as G
    rng = np.random.default_rng(1)
    infos = []
    for s, ts in enumerate((30, 10, 20)):
        key = rng.uniform(-20, 20, (50 + s, 5)).astype(np.float32)
        key.tofile(tmp_path / f"key{s}.bin")
        vel = rng.normal(size=(3, 2))
        vel[1] = np.nan
        infos.append(dict(token=f"t{s}", lidar_path=f"key{s}.bin", timestamp=ts * 1_000_000, gt_boxes=rng.uniform(1, 4, (3, 7)),
                          gt_velocity=vel, gt_names=np.array(["car", "bus", "car"]), valid_flag=np.array([True, False, True]),
                          sweeps=write_sweeps(tmp_path, rng, [20, 30] if s else [], prefix=f"sw{s}_")))
    sc = G.nuscenes_scene(infos[0], str(tmp_path))
    b, src = sc["gt_bboxes_3d"], infos[0]["gt_boxes"].astype(np.float32)
    assert b.dtype == np.float32 and b.shape == (3, 9) and np.array_equal(b[1, 7:], [0, 0])
    assert np.array_equal(b[:, 2], src[:, 2] + src[:, 5] * np.float32(-0.5)) and np.array_equal(b[:, [0, 1, 3, 4, 5, 6]], src[:, [0, 1, 3, 4, 5, 6]])
    assert sc["sample_idx"] == "t0" and sc["valid_flag"].tolist() == [True, False, True] and sc["sweeps_info"]["timestamp"] == 30.0
    scenes = list(G.info_scenes(dict(infos=infos, metadata={}), "nuscenes", str(tmp_path)))
    assert [s["sample_idx"] for s in scenes] == ["t1", "t2", "t0"]                       # sorted by time stamp, as the data set sorts
    assert scenes[2]["sweeps"]["pad"] and not scenes[0]["sweeps"]["pad"] and scenes[0]["sweeps"]["sweeps_num"] == 10
    assert scenes[0]["points"].shape == (51, 5) and len(scenes[0]["sweeps"]["points"]) == 2
    with pytest.raises(ValueError):
        list(G.info_scenes([], "waymo", "."))


def test_entry_points_declared_and_bound():
    """the three new entry points are part of the build (their signatures are pinned in tests/test_abi_cpu.py)"""
    from uni3detr_amd import native as nv
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in ("u3d_gtdb_count", "u3d_gtdb_scan", "u3d_gtdb_crop"):
        assert name in nv.exported_symbols()
    assert os.path.exists(os.path.join(root, "uni3detr_amd", "csrc", "gtdb.hip"))
    src = open(os.path.join(root, "uni3detr_amd", "csrc", "gtdb.hip")).read() + open(os.path.join(root, "uni3detr_amd", "csrc", "point_box.h")).read()
    assert "pb_inside" in src and "atomic" not in src.replace("no atomics", "").replace("No atomics", "")
