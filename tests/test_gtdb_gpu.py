"""The GT-paste database built on the device (uni3detr_amd/csrc/gtdb.hip, uni3detr_amd/gtdb.py) against the NumPy restatement of the
reference's loop (tests/gtdb_ref.py).  Points lie at least 1e-4 from every face plane of every box (the device predicate is f32, the
restatement f64), so the comparison is EXACT: offsets, counts and every output element bit for bit - a copy and one f32 subtraction
have no rounding freedom.  Plus the edge cases and error codes of the entry points, determinism, chunking, the fixed launch count, the
sweep merge in front of the crop, the on-disk round trips, and the database feeding GT-paste into one KITTI training step."""
import ast
import ctypes as C
import os

import numpy as np
import pytest
import torch

import gtdb_ref as R
import sweeps_ref as SR
from test_sweeps_cpu import write_sweeps

pytestmark = pytest.mark.gpu

KITTI = ["Pedestrian", "Cyclist", "Car"]


def _crop(scenes, box_valid=None, n_live=None, max_boxes=None):
    """scenes: [(points, boxes)] host arrays -> native.gtdb_crop's result as host arrays"""
    from uni3detr_amd import native as nv
    lens, gl = [len(p) for p, _ in scenes], [len(b) for _, b in scenes]
    feat, dim = scenes[0][0].shape[1], scenes[0][1].shape[1]
    P = torch.from_numpy(np.concatenate([p for p, _ in scenes]).astype(np.float32).reshape(-1, feat)).cuda()
    B = torch.from_numpy(np.concatenate([b for _, b in scenes]).astype(np.float32).reshape(-1, dim)).cuda()
    so = torch.tensor(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)).cuda()
    bo = torch.tensor(np.concatenate([[0], np.cumsum(gl)]).astype(np.int32)).cuda()
    bv = None if box_valid is None else torch.tensor(np.asarray(box_valid, np.int32)).cuda()
    nl = None if n_live is None else torch.tensor(np.asarray(n_live, np.int32)).cuda()
    out, off, num = nv.gtdb_crop(P, so, nl, max(lens + [0]), B, bo, bv, max_boxes=max_boxes)
    torch.cuda.synchronize()
    return out.cpu().numpy(), off.cpu().numpy(), num.cpu().numpy()


def _check_exact(scenes, got, box_valid=None, n_live=None):
    out, off, num = got
    want = []
    for b, (p, g) in enumerate(scenes):
        want += R.crop_scene(p if n_live is None else p[:n_live[b]], g)
    if box_valid is not None:
        want = [w if v else w[:0] for w, v in zip(want, box_valid)]
    sizes = np.array([len(w) for w in want], np.int64)
    print("objects", len(want), "points", int(sizes.sum()), "empty", int((sizes == 0).sum()))
    assert off.dtype == np.int32 and num.dtype == np.int32 and out.dtype == np.float32
    assert np.array_equal(num, sizes) and np.array_equal(off, np.concatenate([[0], np.cumsum(sizes)]))
    flat = np.concatenate(want) if want else np.zeros((0, out.shape[1]), np.float32)
    assert out.shape == flat.shape and np.array_equal(out.view(np.uint32), flat.astype(np.float32).view(np.uint32))
    return sizes


def test_kitti_shaped_exact(cuda):
    rng = np.random.default_rng(0)
    scenes = [R.random_scene(rng, n, g, 4, 7, extent=40.0) for n, g in ((120_000, 10), (90_000, 14), (300, 3), (110_000, 8))]
    sizes = _check_exact(scenes, _crop(scenes))
    assert sizes.sum() > 20_000


def test_nuscenes_shaped_exact_many_tiles_two_box_blocks(cuda):
    rng = np.random.default_rng(1)
    scenes = [R.random_scene(rng, 300_000, 100, 5, 9), R.random_scene(rng, 40_000, 35, 5, 9), R.random_scene(rng, 270_000, 70, 5, 9)]
    assert len(scenes[0][0]) > 256 * 1024 and len(scenes[0][1]) > 64 and len(scenes[2][1]) > 64
    sizes = _check_exact(scenes, _crop(scenes))
    # overlapping boxes: more object points than points that lie in any box
    in_any = sum(int(R.points_in_rbbox(p[:65536], g[:, :7]).any(1).sum()) for p, g in scenes)
    in_all = sum(int(R.points_in_rbbox(p[:65536], g[:, :7]).sum()) for p, g in scenes)
    assert in_all > in_any > 0 and sizes.sum() > 50_000


@pytest.mark.parametrize("feat", [3, 4, 5, 6, 7, 8])
def test_feature_widths_and_box_widths(cuda, feat):
    rng = np.random.default_rng(10 + feat)
    dim = 7 if feat % 2 else 9
    scenes = [R.random_scene(rng, 3000, 70, feat, dim, extent=15.0), R.random_scene(rng, 700, 5, feat, dim, extent=8.0)]
    _check_exact(scenes, _crop(scenes))


def test_edge_cases(cuda):
    rng = np.random.default_rng(3)
    full, few = R.random_scene(rng, 5000, 20, 4, 7, extent=12.0), R.random_scene(rng, 1000, 6, 4, 7, extent=8.0)
    far = few[1].copy()
    far[:, :2] += 500.0                                      # boxes that hold no point: empty objects, offsets repeat
    no_pts = (np.zeros((0, 4), np.float32), few[1])
    no_box = (few[0], np.zeros((0, 7), np.float32))
    scenes = [no_pts, full, no_box, (few[0], far), few, no_pts]
    sizes = _check_exact(scenes, _crop(scenes))
    assert (sizes[:6] == 0).all() and (sizes[26:32] == 0).all() and sizes[6:26].sum() > 0
    _check_exact([no_pts, no_pts], _crop([no_pts, no_pts]))             # no points at all: every object empty, nothing launched wrongly
    out, off, num = _crop([no_box, no_box])                            # no boxes at all
    assert out.shape == (0, 4) and off.tolist() == [0] and num.shape == (0,)
    valid = (rng.uniform(0, 1, 26) < 0.5).astype(np.int32)
    _check_exact([full, few], _crop([full, few], box_valid=valid), box_valid=valid)
    _check_exact([full, few], _crop([full, few], n_live=[1234, 0]), n_live=[1234, 0])


def test_error_codes_before_any_launch(cuda):
    from uni3detr_amd import native as nv
    rng = np.random.default_rng(4)
    sc = R.random_scene(rng, 500, 4, 4, 7, extent=6.0)
    with pytest.raises(nv.U3DError, match="gtdb_count"):
        _crop([sc], max_boxes=nv.GTDB_MAX_BOXES + 1)
    _crop([sc], max_boxes=nv.GTDB_MAX_BOXES)
    many = (sc[0], np.tile(sc[1], (300, 1)))                            # 1200 boxes in ONE scene: an error, not a truncation
    with pytest.raises(nv.U3DError, match="gtdb_count"):
        _crop([many])
    off = (C.c_int32 * 2)(0, 0)
    UNSUPPORTED = -2
    # int32 offsets: a total of 2^31 rows, or a tile table of 2^31 entries, is refused by the host side of the entry point
    assert nv.lib().u3d_gtdb_crop(None, 0, off, None, 1, 4, 0, None, 0, off, None, 7, 1, None, None, 2 ** 31, None, None) == UNSUPPORTED
    assert nv.lib().u3d_gtdb_count(None, 0, off, None, 1, 4, 2 ** 20, None, 2 ** 11, off, None, 7, 1, None, None) == UNSUPPORTED
    assert nv.lib().u3d_gtdb_count(None, 0, off, None, 1, 9, 0, None, 0, off, None, 7, 1, None, None) == -1        # 9 feature columns
    assert nv.lib().u3d_gtdb_count(None, 0, off, None, 1, 4, 0, None, 0, off, None, 8, 1, None, None) == -1        # 8 box columns


def test_two_runs_identical_bytes(cuda):
    rng = np.random.default_rng(5)
    scenes = [R.random_scene(rng, 60_000, 80, 5, 9, extent=20.0), R.random_scene(rng, 30_000, 30, 5, 9, extent=20.0)]
    a, b = _crop(scenes), _crop(scenes)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and a[0].shape[0] > 10_000


def test_launch_count_does_not_depend_on_scenes_or_boxes(cuda):
    from uni3detr_amd import native as nv
    rng = np.random.default_rng(6)
    small = [R.random_scene(rng, 2000, 1, 4, 7, extent=3.0)]
    big = [R.random_scene(rng, 4000, 100, 4, 7, extent=20.0) for _ in range(8)]
    tags = []
    for scenes in (small, big):
        nv.TIMER = nv.KernelTimer()
        try:
            got = _crop(scenes)
            tags.append([t for t, _ in nv.TIMER.durations_ms()])
        finally:
            nv.TIMER = None
        assert got[2].sum() > 0
    # one bracket per C entry point; u3d_gtdb_count and u3d_gtdb_crop launch one kernel each, u3d_gtdb_scan two (csrc/gtdb.hip)
    assert tags[0] == tags[1] == ["gtdb_count", "gtdb_scan", "gtdb_crop"]


def _dataset(rng, n_scenes, feat=4, dim=7, names=("Car", "Pedestrian", "Cyclist", "Van")):
    out = []
    for s in range(n_scenes):
        g = int(rng.integers(0, 12))
        p, b = R.random_scene(rng, int(rng.integers(2000, 9000)), g, feat, dim, extent=15.0)
        sc = dict(sample_idx=s, points=p, gt_bboxes_3d=b, gt_names=np.asarray(names)[rng.integers(0, len(names), g)])
        if s % 2:
            sc.update(difficulty=rng.integers(-1, 3, g).astype(np.int32), group_ids=rng.integers(0, 4, g), valid_flag=rng.uniform(0, 1, g) < 0.8,
                      score=rng.uniform(0, 1, g).astype(np.float32))
        out.append(sc)
    return out


def _check_infos(got, want):
    assert list(got) == list(want)
    for k in want:
        assert len(got[k]) == len(want[k]), k
        for a, b in zip(got[k], want[k]):
            assert set(a) == set(b)
            for f in b:
                assert np.array_equal(a[f], b[f]), (k, f)


def _check_database(db, infos, objs, feat, classes):
    pts, off = R.key_major(infos, objs, feat)
    assert np.array_equal(db.obj_off.cpu().numpy(), off) and db.obj_off.dtype == torch.int32
    assert np.array_equal(db.points.cpu().numpy().view(np.uint32), pts.view(np.uint32))
    flat = [(k, i) for k, v in infos.items() for i in v]
    assert np.array_equal(db.boxes_host, np.stack([i["box3d_lidar"] for _, i in flat]))
    assert db.labels.tolist() == [classes.index(k) if k in classes else -1 for k, _ in flat]
    assert [(k, len(r)) for k, r in db.rows.items()] == [(k, len(v)) for k, v in infos.items()]


def _same(a, b):
    for f in ("points", "obj_off", "boxes", "labels"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert np.array_equal(a.num_points_in_gt, b.num_points_in_gt) and np.array_equal(a.difficulty, b.difficulty)
    assert list(a.rows) == list(b.rows) and all(np.array_equal(a.rows[k], b.rows[k]) for k in a.rows)
    assert [s._example_num for s in a.samplers.values()] == [s._example_num for s in b.samplers.values()]


@pytest.mark.parametrize("used", [None, ["Car", "Cyclist"]])
def test_database_matches_restatement_and_chunking_does_not_matter(cuda, used):
    from uni3detr_amd import gtdb as G
    scenes = _dataset(np.random.default_rng(7), 9)
    want, objs = R.create_groundtruth_database(scenes, "kitti", used)
    infos1, db1 = G.create_groundtruth_database(iter(scenes), KITTI, info_prefix="kitti", used_classes=used, chunk_scenes=1)
    infos9, db9 = G.create_groundtruth_database(scenes, KITTI, info_prefix="kitti", used_classes=used, chunk_scenes=64)
    infos4, db4 = G.create_groundtruth_database(scenes, KITTI, info_prefix="kitti", used_classes=used, chunk_scenes=4)
    for infos, db in ((infos1, db1), (infos9, db9), (infos4, db4)):
        _check_infos(infos, want)
        _check_database(db, want, objs, 4, KITTI)
    _same(db1, db9)
    _same(db1, db4)
    assert len(db1) > 20 and G.create_groundtruth_database(scenes, KITTI, info_prefix="k", return_database=False)[1] is None


def test_round_trip_from_infos_from_packed_and_returned(cuda, tmp_path):
    from uni3detr_amd import gtdb as G
    scenes = _dataset(np.random.default_rng(8), 6, feat=5, dim=9, names=("car", "bus", "pedestrian"))
    classes = ["car", "pedestrian"]
    infos, db = G.create_groundtruth_database(scenes, classes, info_prefix="nus", out_dir=str(tmp_path), write_points=True,
                                              packed_path=str(tmp_path / "nus.npz"), chunk_scenes=4)
    pkl = tmp_path / "nus_dbinfos_train.pkl"
    assert pkl.exists() and all((tmp_path / i["path"]).exists() for v in infos.values() for i in v)
    assert not (tmp_path / "nus_gt_database" / "img_dir").exists()      # the camera branch is out of scope
    loader = dict(load_dim=5, use_dim=5)
    _same(db, G.GTDatabase.from_infos(str(pkl), str(tmp_path), classes, None, points_loader=loader))
    _same(db, G.GTDatabase.from_packed(str(tmp_path / "nus.npz"), classes))
    prepare = dict(filter_by_difficulty=[-1], filter_by_min_points=dict(car=5, pedestrian=10))
    a = G.GTDatabase.from_infos(str(pkl), str(tmp_path), classes, prepare, points_loader=loader)
    _same(a, G.GTDatabase.from_packed(str(tmp_path / "nus.npz"), classes, prepare))
    assert 0 < len(a) < len(db) and db.box_dim == 9 and db.feat == 5


def test_sweeps_go_through_the_device_merge(cuda, tmp_path):
    from uni3detr_amd import datapath as dp
    from uni3detr_amd import gtdb as G
    rng = np.random.default_rng(9)
    np.random.seed(9)
    ts = 1_533_151_603_547_000 / 1e6
    scenes, host = [], []
    for s, sizes in enumerate(([900, 0, 1500, 700], [], [400] * 12)):
        key = rng.uniform(-30, 30, (8000 + 100 * s, 5)).astype(np.float32)
        key[:, 2] = rng.uniform(-3, 4, len(key)).astype(np.float32)   # the key frame at the boxes' height, so that objects hold points
        info = dict(timestamp=ts + s, sweeps=write_sweeps(tmp_path, rng, sizes, prefix=f"b{s}_"))
        rec = dp.read_sweeps(info, G.SWEEPS_ENTRY)
        e = G.SWEEPS_ENTRY
        merged = SR.load_points_from_multi_sweeps(key, info["sweeps"], info["timestamp"], e["sweeps_num"], e["load_dim"], e["use_dim"],
                                                  e["pad_empty_sweeps"], e["remove_close"], False,
                                                  choices=rec["choices"] if not rec["pad"] else None, explicit=True)[0]
        _, boxes = R.random_scene(rng, 0, 60, 5, 9, extent=25.0)
        boxes = boxes[(R.face_distance(merged, boxes) >= 1e-4).all(0)]  # keep the boxes no merged point comes close to a face of
        assert len(boxes) > 15
        names = np.asarray(["car", "truck", "bus"])[rng.integers(0, 3, len(boxes))]
        scenes.append(dict(sample_idx=f"tok{s}", points=key, gt_bboxes_3d=boxes, gt_names=names, sweeps=rec))
        host.append(dict(sample_idx=f"tok{s}", points=merged, gt_bboxes_3d=boxes, gt_names=names))
    assert scenes[1]["sweeps"]["pad"] and len(scenes[2]["sweeps"]["choices"]) == 10
    want, objs = R.create_groundtruth_database(host, "nus")
    infos, db = G.create_groundtruth_database(scenes, ["car", "truck", "bus"], info_prefix="nus", chunk_scenes=2)
    _check_infos(infos, want)
    _check_database(db, want, objs, 5, ["car", "truck", "bus"])
    assert int(db.obj_off_host[-1]) > 100


def test_built_database_feeds_gt_paste_into_a_kitti_training_step(cuda):
    import projects.mmdet3d_plugin  # noqa: F401
    import test_objaug_gpu as T
    from uni3detr_amd import datapath as dp
    from uni3detr_amd import gtdb as G
    from uni3detr_amd.registry import build_model, to_config
    from uni3detr_amd.trainer import TrainStep
    rng = np.random.default_rng(21)
    np.random.seed(21)
    torch.manual_seed(0)
    src = []
    for s in range(4):                                      # source scenes: 20 well separated objects each, as test_objaug_gpu builds them
        gx, gy = np.meshgrid(np.arange(5) * 12.0 + 6, np.arange(4) * 16.0 - 24)
        b, lab = T._boxes(rng, 20)
        b[:, 0], b[:, 1] = gx.ravel() + rng.uniform(-1, 1, 20), gy.ravel() + rng.uniform(-1, 1, 20)
        bg = np.stack([rng.uniform(0, 70, 3000), rng.uniform(-40, 40, 3000), rng.uniform(-3, 1, 3000), rng.uniform(0, 1, 3000)], 1)
        pts = np.concatenate([T._inside(rng, bb, int(rng.integers(5, 60))) for bb in b] + [T._clear_of_faces(bg, b).astype(np.float32)])
        src.append(dict(sample_idx=s, points=pts, gt_bboxes_3d=b, gt_names=np.asarray(T.CLASSES)[lab]))
    infos, db = G.create_groundtruth_database(src, T.CLASSES, info_prefix="kitti", chunk_scenes=3)
    want, objs = R.create_groundtruth_database(src, "kitti")
    _check_infos(infos, want)
    _check_database(db, want, objs, 4, T.CLASSES)
    assert len(db) == 80 and set(db.rows) == set(T.CLASSES) and min(db.num_points_in_gt) >= 5
    pipe = dp.DevicePipeline(T._kitti_pipeline(), gt_database=db, object_noise=True)
    assert [type(t).__name__ for t in pipe.transforms][:2] == ["ObjectSample", "ObjectNoise"]
    scenes = T._scenes(rng, db, [(30000, 10), (25000, 4)])
    n_gt = sum(len(b) for _, b, _ in scenes)
    batch = pipe(T._batch(scenes))
    pts, gts, labels = dp.unpack_batch(batch)
    assert [int(p.shape[0]) for p in pts] == [18000, 18000]
    assert sum(int(l.shape[0]) for l in labels) > n_gt                 # objects of the new database were pasted and survived the filter
    shipped = os.path.join(os.path.dirname(__file__), "golden", "shipped_configs.txt")
    model = build_model(to_config(ast.literal_eval(open(shipped).read())["kitti_3classes"]["config"]["model"])).to(cuda).train()
    model.set_precision("bf16")
    loss = float(TrainStep(model, pts, gts, labels, graph=False, lr=1e-4).step())
    assert np.isfinite(loss) and loss > 0
