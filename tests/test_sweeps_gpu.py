"""LoadPointsFromMultiSweeps, PointShuffle and ObjectNameFilter on the device (uni3detr_amd/csrc/sweeps.hip, datapath.hip) against the
loop-by-loop restatement (tests/sweeps_ref.py): the sweep merge bit for bit (the restatement in the device's explicit summation order),
the shuffle's permutation properties, the name filter after ObjectRangeFilter, and the nuScenes train pipeline end to end into one
training step."""
import ast
import copy
import os

import numpy as np
import pytest
import torch

import sweeps_ref as R
from test_sweeps_cpu import ENTRY, write_sweeps

pytestmark = pytest.mark.gpu

TS = 1_533_151_603_547_000 / 1e6
BOUNDARY = np.array([[1, 0.5], [-1, 0.5], [0.5, 1], [0.5, -1], [1, 1], [-1, -1], [0.99999994, 0.99999994], [-0.99999994, 0.99999994],
                     [1.0000001, 0.2], [0, 0], [0.2, -1.0000001]], np.float32)


def _key(rng, n, load_dim=5):
    k = rng.uniform(-40, 40, (n, load_dim)).astype(np.float32)
    k[: n // 10, :2] = rng.uniform(-1.5, 1.5, (n // 10, 2)).astype(np.float32)
    m = min(n, len(BOUNDARY))
    k[:m, :2] = BOUNDARY[:m]
    return k


def _with_boundary(sweeps, rng, load_dim=5):
    """rewrite every non-empty sweep file with the |x| = 1 / |y| = 1 boundary rows at its front"""
    for sw in sweeps:
        a = np.fromfile(sw["data_path"], np.float32).reshape(-1, load_dim)
        m = min(len(a), len(BOUNDARY))
        a[:m, :2] = BOUNDARY[:m]
        a.tofile(sw["data_path"])
    return sweeps


def _merge(tmp_path, spec, entry, seed=0):
    """spec: per scene (key rows, [sweep file rows]) -> (device batch after the merge, restated scenes, records)."""
    from uni3detr_amd import datapath as dp
    rng = np.random.default_rng(seed)
    ld = entry.get("load_dim", 5)
    keys, infos = [], []
    for b, (n, sizes) in enumerate(spec):
        keys.append(_key(rng, n, ld))
        infos.append(dict(timestamp=TS + b, sweeps=_with_boundary(write_sweeps(tmp_path, rng, sizes, ld, prefix=f"b{b}_"), rng, ld)))
    np.random.seed(seed)
    recs = [dp.read_sweeps(info, entry) for info in infos]
    batch = dp.pack_batch([torch.from_numpy(k).cuda() for k in keys], box_type_3d="LiDAR", sweeps=recs)
    batch = dp.DevicePipeline([entry], sweeps=True)(batch)
    e = dp.OBJECT_AUG.build(entry)
    ref = [R.load_points_from_multi_sweeps(k, info["sweeps"], info["timestamp"], e.sweeps_num, e.load_dim, e.use_dim, e.pad_empty_sweeps,
                                           e.remove_close, e.test_mode, choices=rec["choices"] if not rec["pad"] else None, explicit=True)[0]
           for k, info, rec in zip(keys, infos, recs)]
    return batch, ref, recs


def _check_merge(batch, ref):
    so = batch["scene_off"].cpu().numpy()
    ref_off = np.concatenate([[0], np.cumsum([len(r) for r in ref])])
    assert np.array_equal(so, ref_off), (so, ref_off)
    pts = batch["points"].cpu().numpy()
    assert pts.shape[0] >= ref_off[-1] and pts.shape[1] == ref[0].shape[1]
    for b, r in enumerate(ref):
        got = pts[so[b]:so[b + 1]]
        assert np.array_equal(got.view(np.int32), r.view(np.int32)), (b, np.argwhere(got != r)[:5])


CASES = {
    "one_scene_more_sweeps": ([(1000, [300, 513, 0, 256, 700, 1, 90, 400, 257, 600, 33, 255])], {}),
    "two_scenes_fewer_and_more": ([(777, [100, 200, 300]), (256, [50] * 11)], {}),
    "three_scenes_empty_files_use_dim": ([(500, [0, 0, 129]), (0, [40, 0]), (1023, [512, 0, 1025, 3])], dict(use_dim=[0, 1, 2, 4])),
    "four_scenes_padding": ([(700, []), (300, [10, 20]), (0, []), (257, [300] * 10)], {}),
    "four_scenes_no_padding": ([(700, []), (300, [10, 20]), (0, []), (257, [300] * 10)], dict(pad_empty_sweeps=False)),
    "no_remove_close_test_mode": ([(640, [70] * 12), (90, [])], dict(remove_close=False, test_mode=True, use_dim=[4, 0, 1])),
    "empty_first_middle_last_segment": ([(0, [0, 40]), (120, [0, 60, 0]), (50, [30, 0])], {}),
    "load_dim_6": ([(400, [200, 0, 300])], dict(load_dim=6, use_dim=[0, 1, 2, 5, 4], sweeps_num=2)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_sweep_merge_matches_restatement(cuda, tmp_path, case):
    spec, over = CASES[case]
    entry = dict(ENTRY, **over)
    batch, ref, recs = _merge(tmp_path, spec, entry, seed=len(case))
    _check_merge(batch, ref)
    assert batch["sweep_choices"] is not None and len(batch["sweep_choices"]) == len(spec)


def test_sweep_merge_large_scene(cuda, tmp_path):
    spec = [(34_720, [34_700 + 13 * j for j in range(12)]), (5000, [4000] * 3)]
    batch, ref, _ = _merge(tmp_path, spec, ENTRY, seed=9)
    assert len(ref[0]) >= 300_000
    _check_merge(batch, ref)


def test_sweep_merge_then_range_filter(cuda, tmp_path):
    """PointsRangeFilter runs unchanged on the merged batch (spare rows past scene_off[-1] untouched)."""
    from uni3detr_amd import datapath as dp
    batch, ref, _ = _merge(tmp_path, [(3000, [2000] * 4), (1000, [500] * 2)], ENTRY, seed=4)
    rf = dp.PointsRangeFilter([-20, -20, -5, 20, 20, 3])
    batch = rf(batch)
    so, cnt = batch["scene_off"].cpu().numpy(), batch["count"].cpu().numpy()
    pts = batch["points"].cpu().numpy()
    for b, r in enumerate(ref):
        keep = (r[:, 0] > -20) & (r[:, 1] > -20) & (r[:, 2] > -5) & (r[:, 0] < 20) & (r[:, 1] < 20) & (r[:, 2] < 3)
        assert cnt[b] == keep.sum() and np.array_equal(pts[so[b]:so[b] + cnt[b]], r[keep])


def _shuffle_batch(spec, seed=0):
    rng = np.random.default_rng(seed)
    pts = np.concatenate([np.stack([np.arange(n, dtype=np.float32) + 1000 * b, rng.uniform(0, 1, n).astype(np.float32),
                                    np.full(n, b, np.float32)], 1) for b, n in enumerate(spec)])
    off = np.concatenate([[0], np.cumsum(spec)]).astype(np.int32)
    return torch.from_numpy(pts).cuda(), torch.from_numpy(off).cuda(), pts, off


def test_point_shuffle_permutes_live_rows_within_their_scene(cuda):
    from uni3detr_amd import datapath as dp
    from uni3detr_amd import native as nv
    spec = [1000, 1, 0, 777, 4096]
    p, so, p_h, off = _shuffle_batch(spec)
    count = torch.tensor([1000, 1, 0, 500, 4000], dtype=torch.int32, device=cuda)
    seed = torch.tensor([12345], dtype=torch.int64, device=cuda)
    a = nv.point_shuffle(p, so, count, seed).cpu().numpy()
    b = nv.point_shuffle(p, so, count, seed).cpu().numpy()
    assert np.array_equal(a, b)                                             # the same seed reproduces
    cnt = count.cpu().numpy()
    moved = 0
    for s in range(len(spec)):
        seg, out = p_h[off[s]:off[s + 1]], a[off[s]:off[s + 1]]
        live = cnt[s]
        assert np.array_equal(np.sort(out[:live, 0]), seg[:live, 0])       # an exact permutation of the live rows ...
        assert np.array_equal(out[:live][np.argsort(out[:live, 0])], seg[:live])
        assert np.array_equal(out[live:], seg[live:])                      # ... the dead rows untouched
        moved += int((out[:live, 0] != seg[:live, 0]).sum())
    assert moved > 0.9 * sum(cnt)
    # whole segments without count; the DevicePipeline entry advances its seed on every call
    batch = dict(points=p.clone(), scene_off=so)
    sh = dp.PointShuffle()
    np.random.seed(1)
    first = sh(dict(batch))["points"].cpu().numpy()
    second = sh(dict(batch))["points"].cpu().numpy()
    assert not np.array_equal(first, second)
    for out in (first, second):
        for s in range(len(spec)):
            assert np.array_equal(np.sort(out[off[s]:off[s + 1], 0]), p_h[off[s]:off[s + 1], 0])


def test_point_shuffle_is_the_declared_keyed_permutation(cuda):
    """row k of scene b's live prefix comes from row feistel_perm(k, n, key(seed, b)) (tests/sweeps_ref.py), exactly"""
    from uni3detr_amd import native as nv
    spec = [37, 1, 300, 64]
    p, so, p_h, off = _shuffle_batch(spec, seed=2)
    count = torch.tensor([37, 1, 250, 64], dtype=torch.int32, device=cuda)
    for sd in (0, 987654321987, -7):
        out = nv.point_shuffle(p, so, count, torch.tensor([sd], dtype=torch.int64, device=cuda)).cpu().numpy()
        for b, n in enumerate(count.tolist()):
            key = R.shuffle_key(sd, b)
            src = [R.feistel_perm(k, n, key) for k in range(n)]
            assert np.array_equal(out[off[b]:off[b] + n], p_h[off[b] + np.array(src, np.int64)]), (sd, b)


def test_point_shuffle_position_frequencies(cuda):
    """4096 seeds over one 10-row scene: every (position, row) pair within a loose band around 4096 / 10 (deterministic)."""
    from uni3detr_amd import native as nv
    n = 10
    p, so, _, _ = _shuffle_batch([n])
    hits = torch.zeros((n, n), dtype=torch.int64, device=cuda)
    seeds = torch.arange(4096, dtype=torch.int64, device=cuda) * 0x2545F4914F6CDD1D
    pos = torch.arange(n, device=cuda)
    for k in range(4096):
        out = nv.point_shuffle(p, so, None, seeds[k:k + 1].contiguous())
        hits[pos, out[:, 0].long()] += 1
    h = hits.cpu().numpy()
    assert np.all(h.sum(0) == 4096) and np.all(h.sum(1) == 4096)
    e = 4096 / n
    assert h.min() > 0.6 * e and h.max() < 1.4 * e, (h.min() / e, h.max() / e)


@pytest.mark.parametrize("dim", [7, 9])
def test_object_name_filter_after_range_filter(cuda, dim):
    from uni3detr_amd import datapath as dp
    rng = np.random.default_rng(dim)
    classes = ["car", "truck", "bus", "pedestrian"]
    sizes = [0, 1, 70, 130, 5]
    boxes, labels = [], []
    for g in sizes:
        b = np.zeros((g, dim), np.float32)
        b[:, :2] = rng.uniform(-60, 60, (g, 2))
        b[:, 3:6] = rng.uniform(0.5, 4, (g, 3))
        b[:, 6] = rng.uniform(-np.pi, np.pi, g)
        if dim == 9:
            b[:, 7:] = rng.normal(size=(g, 2))
        boxes.append(b)
        labels.append(rng.integers(-1, 6, g).astype(np.int32))
    batch = dp.pack_batch([torch.zeros((4, 5), device=cuda)] * len(sizes), [torch.from_numpy(b).cuda() for b in boxes], "LiDAR",
                          gt_labels_3d=[torch.from_numpy(l).cuda() for l in labels])
    rng_f = [-54, -54, -5.0, 54, 54, 3.0]
    batch = dp.DevicePipeline([dict(type="ObjectRangeFilter", point_cloud_range=rng_f), dict(type="ObjectNameFilter", classes=classes)],
                              name_filter=True)(batch)
    go, gc = batch["gt_off"].cpu().numpy(), batch["gt_count"].cpu().numpy()
    got_b, got_l = batch["gt_bboxes_3d"].cpu().numpy(), batch["gt_labels_3d"].cpu().numpy()
    for s, (b, l) in enumerate(zip(boxes, labels)):
        keep = (b[:, 0] > -54) & (b[:, 1] > -54) & (b[:, 0] < 54) & (b[:, 1] < 54)
        rb, rl = R.object_name_filter(b[keep], l[keep], classes)
        assert gc[s] == len(rl)
        assert np.array_equal(got_l[go[s]:go[s] + gc[s]], rl)
        exp = rb.copy()
        exp[:, 6] = exp[:, 6] - np.floor(exp[:, 6] / np.float32(6.283185307179586) + np.float32(0.5)) * np.float32(6.283185307179586)
        np.testing.assert_allclose(got_b[go[s]:go[s] + gc[s]], exp, rtol=0, atol=1e-6)
        assert np.array_equal(got_b[go[s]:go[s] + gc[s], :6], rb[:, :6])
    # without ObjectRangeFilter the whole segment is the live prefix
    batch = dp.pack_batch([torch.zeros((4, 5), device=cuda)] * len(sizes), [torch.from_numpy(b).cuda() for b in boxes], "LiDAR",
                          gt_labels_3d=[torch.from_numpy(l).cuda() for l in labels])
    batch = dp.OBJECT_AUG.build(dict(type="ObjectNameFilter", classes=classes))(batch)
    gc = batch["gt_count"].cpu().numpy()
    assert list(gc) == [int(((l >= 0) & (l < 4)).sum()) for l in labels]


def test_sweep_merge_then_test_time_augmentation(cuda, tmp_path):
    """A MultiScaleFlipAug3D entry after the merge expands the merged scenes, spare rows past scene_off[-1] included, exactly as it
    expands the same scenes packed without spare rows."""
    from uni3detr_amd import datapath as dp
    entry = dict(ENTRY, test_mode=True)
    batch, ref, _ = _merge(tmp_path, [(3000, [2000] * 11), (700, []), (1500, [900, 0, 1100])], entry, seed=12)
    assert batch["points"].shape[0] > int(batch["scene_off"][-1])           # remove_close left spare rows
    assert "sweeps" not in batch and "sweep_choices" in batch               # the device tables are dropped after the merge
    tta = dict(type="MultiScaleFlipAug3D", flip=True, pcd_horizontal_flip=True, pcd_vertical_flip=True,
               transforms=[dict(type="RandomFlip3D", sync_2d=False),
                           dict(type="PointsRangeFilter", point_cloud_range=[-25, -25, -5, 25, 25, 3])])
    out = dp.DevicePipeline([tta])(batch)
    packed = dp.DevicePipeline([tta])(dp.pack_batch([torch.from_numpy(r).cuda() for r in ref], box_type_3d="LiDAR"))
    assert out["tta_views"] == 4 and torch.equal(out["scene_off"], packed["scene_off"]) and torch.equal(out["count"], packed["count"])
    a, h = dp.unpack_batch(out)[0], dp.unpack_batch(packed)[0]
    assert len(a) == 12
    for x, y in zip(a, h):
        assert torch.equal(x, y)


# ---- the nuScenes train pipeline end to end ----
NUSC_CLASSES = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone"]


def _nusc_pipeline(shuffle=True):
    from uni3detr_amd.configs import pipelines as P
    cfg = copy.deepcopy(P.SHIPPED["nuscenes"]["train_pipeline"])
    out = []
    for c in cfg:
        if c["type"] == "LoadPointsFromMultiSweeps":
            c.update(ENTRY)
        if c["type"] == "ObjectSample":
            c["db_sampler"] = dict(type="UnifiedDataBaseSampler", rate=1.0, classes=NUSC_CLASSES,
                                   sample_groups=dict(car=2, truck=3, bus=4, pedestrian=2, traffic_cone=2))
        if c["type"] == "ObjectNameFilter":
            c["classes"] = NUSC_CLASSES
        if c["type"] == "PointShuffle" and not shuffle:
            continue
        out.append(c)
    return out


def _nusc_scenes(tmp_path, rng):
    """two nuScenes-shaped scenes (smaller): key frames, sweep files, 9-column boxes, labels with some -1 (names outside classes)."""
    scenes = []
    for b, (n, ns, g) in enumerate([(6000, 12, 9), (3000, 0, 5)]):
        key = rng.uniform(-50, 50, (n, 5)).astype(np.float32)
        key[:, 2] = rng.uniform(-4, 2, n)
        sw = write_sweeps(tmp_path, rng, [int(v) for v in rng.integers(500, 3000, ns)], prefix=f"n{b}_")
        box = np.zeros((g, 9), np.float32)
        box[:, :2] = rng.uniform(-58, 58, (g, 2))
        box[:, 2] = -1.5
        box[:, 3:6] = rng.uniform(0.6, 4.5, (g, 3))
        box[:, 6] = rng.uniform(-np.pi, np.pi, g)
        box[:, 7:] = rng.normal(size=(g, 2))
        lab = rng.integers(-1, 10, g).astype(np.int32)
        scenes.append((key, dict(timestamp=TS + b, sweeps=sw), box, lab))
    return scenes


def _nusc_database(rng):
    from uni3detr_amd.gtdb import GTDatabase
    P_, G, L = [], [], []
    for s in range(3):
        g = 12
        box = np.zeros((g, 9), np.float32)
        gx, gy = np.meshgrid(np.arange(4) * 12.0 - 18, np.arange(3) * 12.0 - 12)
        box[:, 0], box[:, 1], box[:, 2] = gx.ravel(), gy.ravel(), -1.5
        box[:, 3:6] = rng.uniform(0.8, 3.0, (g, 3))
        lab = np.array([0, 1, 3, 8, 9] * 3)[:g].astype(np.int64)
        pts = []
        for bb in box:
            q = rng.uniform(-0.45, 0.45, (30, 3)) * bb[3:6] + np.array([0, 0, 0.5]) * bb[3:6] + bb[:3]
            pts.append(np.concatenate([q, rng.uniform(0, 1, (30, 2))], 1).astype(np.float32))
        P_.append(torch.from_numpy(np.concatenate(pts)).cuda())
        G.append(torch.from_numpy(box).cuda())
        L.append(torch.from_numpy(lab).cuda())
    return GTDatabase.from_scenes(P_, G, L, NUSC_CLASSES)


def _nusc_run(tmp_path, shuffle=True):
    from uni3detr_amd import datapath as dp
    rng = np.random.default_rng(31)
    np.random.seed(31)
    db = _nusc_database(rng)
    scenes = _nusc_scenes(tmp_path, rng)
    pipe = dp.DevicePipeline(_nusc_pipeline(shuffle), gt_database=db, sweeps=True, point_shuffle=True, name_filter=True)
    entry = dict(ENTRY)
    recs = [dp.read_sweeps(info, entry) for _, info, _, _ in scenes]
    batch = dp.pack_batch([torch.from_numpy(k).cuda() for k, _, _, _ in scenes], [torch.from_numpy(g).cuda() for _, _, g, _ in scenes],
                          "LiDAR", gt_labels_3d=[torch.from_numpy(l).cuda() for _, _, _, l in scenes], sweeps=recs)
    return pipe, pipe(batch), scenes, db


def test_nuscenes_pipeline_matches_host_merge_and_name_filter(cuda, tmp_path):
    """Without PointShuffle: the device pipeline with all opt-ins equals the same pipeline fed the host-restated merge, with the
    restated ObjectNameFilter applied to its boxes (every draw replayed from the first run's batch)."""
    from uni3detr_amd import datapath as dp
    pipe, out, scenes, db = _nusc_run(tmp_path, shuffle=False)
    names = [type(t).__name__ for t in pipe.transforms]
    assert names[0] == "LoadPointsFromMultiSweeps" and "ObjectNameFilter" in names and not pipe.skipped.count("PointShuffle")
    merged = [R.load_points_from_multi_sweeps(k, info["sweeps"], info["timestamp"], 9, 5, [0, 1, 2, 3, 4], True, True,
                                              choices=c if len(info["sweeps"]) else None, explicit=True)[0]
              for (k, info, _, _), c in zip(scenes, out["sweep_choices"])]
    host_cfg = [c for c in _nusc_pipeline(False) if c["type"] not in ("LoadPointsFromMultiSweeps", "ObjectNameFilter")]
    host_pipe = dp.DevicePipeline(host_cfg, gt_database=db)
    hb = dp.pack_batch([torch.from_numpy(m).cuda() for m in merged], [torch.from_numpy(g).cuda() for _, _, g, _ in scenes], "LiDAR",
                       gt_labels_3d=[torch.from_numpy(l).cuda() for _, _, _, l in scenes])
    for k in ("db_sampled", "pcd_rotation_angle", "pcd_scale_factor", "pcd_horizontal_flip", "pcd_vertical_flip", "pcd_trans"):
        hb[k] = out[k]
    hb = host_pipe(hb)
    dp_pts, dp_box, dp_lab = dp.unpack_batch(out)
    h_pts, h_box, h_lab = dp.unpack_batch(hb)
    for b in range(len(scenes)):
        a, h = dp_pts[b].cpu().numpy(), h_pts[b].cpu().numpy()
        assert a.shape == h.shape and a.shape[0] > 1000
        assert np.array_equal(a[np.lexsort(a.T[::-1])], h[np.lexsort(h.T[::-1])])           # the same point multiset
        rb, rl = R.object_name_filter(h_box[b].tensor.cpu().numpy(), h_lab[b].cpu().numpy(), NUSC_CLASSES)
        assert np.array_equal(dp_box[b].tensor.cpu().numpy(), rb) and np.array_equal(dp_lab[b].cpu().numpy(), rl)
        assert (dp_lab[b].cpu().numpy() >= 0).all()


def test_nuscenes_pipeline_into_a_training_step(cuda, tmp_path):
    import projects.mmdet3d_plugin  # noqa: F401
    from uni3detr_amd import datapath as dp
    from uni3detr_amd.registry import build_model, to_config
    from uni3detr_amd.trainer import TrainStep
    torch.manual_seed(0)
    pipe, out, scenes, _ = _nusc_run(tmp_path, shuffle=True)
    assert "PointShuffle" in [type(t).__name__ for t in pipe.transforms] and not pipe.skipped.count("LoadPointsFromMultiSweeps")
    pts, gts, labels = dp.unpack_batch(out)
    assert all(int(g.tensor.shape[0]) == int(l.shape[0]) for g, l in zip(gts, labels))
    assert all((l >= 0).all() for l in labels)
    shipped = os.path.join(os.path.dirname(__file__), "golden", "shipped_configs.txt")
    model = build_model(to_config(ast.literal_eval(open(shipped).read())["nuscenes"]["config"]["model"])).to(cuda).train()
    model.set_precision("bf16")
    ts = TrainStep(model, pts, gts, labels, graph=False, lr=1e-4)
    loss = float(ts.step())
    assert np.isfinite(loss) and loss > 0


def test_new_steps_make_no_device_to_host_copy(cuda, tmp_path):
    from uni3detr_amd import datapath as dp
    rng = np.random.default_rng(3)
    keys = [_key(rng, 2000), _key(rng, 500)]
    infos = [dict(timestamp=TS, sweeps=write_sweeps(tmp_path, rng, [400] * 11)), dict(timestamp=TS, sweeps=[])]
    recs = [dp.read_sweeps(i, ENTRY) for i in infos]
    boxes = [torch.from_numpy(rng.uniform(-10, 10, (6, 9)).astype(np.float32)).cuda() for _ in keys]
    labels = [torch.tensor([0, -1, 3, 12, 2, 1], dtype=torch.int32, device=cuda) for _ in keys]
    batch = dp.pack_batch([torch.from_numpy(k).cuda() for k in keys], boxes, "LiDAR", gt_labels_3d=labels, sweeps=recs)
    merge = dp.OBJECT_AUG.build(ENTRY)
    shuffle = dp.OBJECT_AUG.build(dict(type="PointShuffle"))
    names = dp.OBJECT_AUG.build(dict(type="ObjectNameFilter", classes=NUSC_CLASSES))
    rf = dp.PointsRangeFilter([-54, -54, -5.0, 54, 54, 3.0])
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        batch = merge(batch)
        batch = rf(batch)
        batch = shuffle(batch)
        batch = shuffle(batch)
        batch = names(batch)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert batch["gt_count"].tolist() == [4, 4]
    assert int(batch["count"].sum()) > 0
