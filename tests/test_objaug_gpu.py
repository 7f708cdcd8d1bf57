"""GT-paste (ObjectSample / UnifiedObjectSample) and ObjectNoise on the device (uni3detr_amd/csrc/objaug.hip) against the NumPy
restatement of the upstream helpers (tests/objaug_ref.py), fed the draws the device path recorded in the batch dict; plus the draws
themselves, edge cases, the opt-in of DevicePipeline and the KITTI 3-class train pipeline end to end into one training step.
Points are generated at least 1e-4 from every face of every box: no boundary cases."""
import ast
import copy
import os

import numpy as np
import pytest
import torch

import objaug_ref as R

pytestmark = pytest.mark.gpu

CLASSES = ["Car", "Pedestrian", "Cyclist"]
SIZES = [(3.9, 1.6, 1.5), (0.8, 0.6, 1.7), (1.8, 0.6, 1.7)]
RANGE = [0, -40, -3, 70.4, 40, 1]
DB_SAMPLER = dict(rate=1.0, classes=CLASSES, sample_groups=dict(Car=15, Pedestrian=6, Cyclist=6))
MARGIN = 1e-4


def _boxes(rng, n, lo=(2, -36), hi=(68, 36)):
    lab = rng.integers(0, 3, n)
    b = np.zeros((n, 7), np.float32)
    b[:, 0], b[:, 1], b[:, 2] = rng.uniform(lo[0], hi[0], n), rng.uniform(lo[1], hi[1], n), rng.uniform(-2, -1, n)
    b[:, 3:6] = np.array(SIZES, np.float32)[lab] * rng.uniform(0.9, 1.1, (n, 1))
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    return b, lab


def _inside(rng, box, m):
    """m points strictly inside the box, at least MARGIN * 10 from its faces."""
    q = rng.uniform(-0.49, 0.49, (m, 3)) * box[3:6] + np.array([0, 0, 0.5]) * box[3:6]
    c, s = np.cos(box[6]), np.sin(box[6])
    p = np.stack([q[:, 0] * c - q[:, 1] * s + box[0], q[:, 0] * s + q[:, 1] * c + box[1], q[:, 2] + box[2], rng.uniform(0, 1, m)], 1)
    return p.astype(np.float32)


def _clear_of_faces(p, boxes):
    """drop the points closer than MARGIN to a face plane of any box (float64, the restatement's frame)."""
    keep = np.ones(len(p), bool)
    for b in np.asarray(boxes, np.float64):
        dx, dy = p[:, 0] - b[0], p[:, 1] - b[1]
        c, s = np.cos(b[6]), np.sin(b[6])
        lx, ly = dx * c + dy * s, -dx * s + dy * c
        for d in (np.abs(np.abs(lx) - b[3] / 2), np.abs(np.abs(ly) - b[4] / 2), np.abs(p[:, 2] - b[2]), np.abs(p[:, 2] - b[2] - b[5])):
            keep &= d >= MARGIN
    return p[keep]


def _database(rng, n_obj=120, cyclists=3):
    """GTDatabase.from_scenes over source scenes of well separated boxes; Cyclist kept small so its sampler wraps."""
    from uni3detr_amd.gtdb import GTDatabase
    P, G, L = [], [], []
    left = n_obj
    while left > 0:
        n = min(20, left)
        gx, gy = np.meshgrid(np.arange(5) * 12.0 + 6, np.arange(4) * 16.0 - 24)
        b, lab = _boxes(rng, n)
        b[:, 0], b[:, 1] = gx.ravel()[:n] + rng.uniform(-1, 1, n), gy.ravel()[:n] + rng.uniform(-1, 1, n)
        pts = [_inside(rng, bb, int(rng.integers(5, 60))) for bb in b]
        bg = np.stack([rng.uniform(0, 70, 3000), rng.uniform(-40, 40, 3000), rng.uniform(-3, 1, 3000), rng.uniform(0, 1, 3000)], 1)
        P.append(torch.from_numpy(np.concatenate(pts + [_clear_of_faces(bg, b).astype(np.float32)])).cuda())
        G.append(torch.from_numpy(b).cuda())
        L.append(torch.from_numpy(lab).cuda())
        left -= n
    lab_all = torch.cat(L)
    cyc = torch.nonzero(lab_all == 2).flatten()
    lab_all[cyc[cyclists:]] = 0               # only `cyclists` Cyclist objects remain
    L = list(torch.split(lab_all, [int(g.shape[0]) for g in G]))
    return GTDatabase.from_scenes(P, G, L, CLASSES)


def _scenes(rng, db, spec):
    """spec: list of (n_points, n_gt); points kept clear of every GT and database face."""
    out = []
    for n, g in spec:
        b, lab = _boxes(rng, g)
        lab[lab == 2] = 1 if len(out) % 2 else 2           # a scene without Cyclists every other scene
        p = np.stack([rng.uniform(0, 70, n), rng.uniform(-40, 40, n), rng.uniform(-3, 1, n), rng.uniform(0, 1, n)], 1)
        p = _clear_of_faces(p, np.concatenate([b, db.boxes_host]))
        pts = np.concatenate([p.astype(np.float32)] + [_inside(rng, bb, 15) for bb in b])
        out.append((pts, b, lab))
    return out


def _batch(scenes):
    from uni3detr_amd import datapath as dp
    return dp.pack_batch([torch.from_numpy(p).cuda() for p, _, _ in scenes], [torch.from_numpy(b).cuda() for _, b, _ in scenes], "LiDAR",
                         gt_labels_3d=[torch.from_numpy(l).cuda() for _, _, l in scenes])


def _split(batch):
    so, go = batch["scene_off"].tolist(), batch["gt_off"].tolist()
    P, G, L = batch["points"].cpu().numpy(), batch["gt_bboxes_3d"].cpu().numpy(), batch["gt_labels_3d"].cpu().numpy()
    return [(P[so[b]:so[b + 1]], G[go[b]:go[b + 1]], L[go[b]:go[b + 1]]) for b in range(len(so) - 1)]


def _host_draws(seed_state, db, scenes):
    """the draws of the restatement: the same shuffles (one BatchSampler per class, in class order), sample_all's sampled_num."""
    np.random.set_state(seed_state)
    samp = {c: R.BatchSampler(list(range(int(np.sum(db.labels.cpu().numpy() == i)))), c) for i, c in enumerate(CLASSES)}
    draws = []
    for _, _, lab in scenes:
        rows, grp = [], []
        for gi, (name, mx) in enumerate(DB_SAMPLER["sample_groups"].items()):
            n = int(np.round(1.0 * int(mx - np.sum(lab == CLASSES.index(name)))))
            if n > 0:
                r = db.rows[name][np.asarray(samp[name].sample(n), np.int64)]
                rows += list(r)
                grp += [gi] * len(r)
        draws.append((np.array(rows, np.int64), np.array(grp, np.int64)))
    return draws


def _restated_paste(scenes, db, draws, sampled_first):
    pts_h, off = db.points.cpu().numpy(), db.obj_off_host
    lab_h = db.labels.cpu().numpy()
    return [R.paste_scene(p.astype(np.float64), g.astype(np.float64), l, db.boxes_host[rows], lab_h[rows],
                          [pts_h[off[r]:off[r + 1]] for r in rows], grp, sampled_first) for (p, g, l), (rows, grp) in zip(scenes, draws)]


@pytest.mark.parametrize("kind", ["ObjectSample", "UnifiedObjectSample"])
def test_object_sample_matches_restatement(cuda, kind):
    from uni3detr_amd import datapath as dp
    rng = np.random.default_rng(1 if kind == "ObjectSample" else 2)
    np.random.seed(5)
    state = np.random.get_state()            # the database's samplers shuffle first, then the transform draws
    db = _database(rng)
    big = np.array([[35, 0, -3, 200, 200, 6, 0]], np.float32)
    scenes = _scenes(rng, db, [(20000, 6), (15000, 0), (30000, 12), (8000, 3)])
    p_all, _, _ = scenes[3]
    scenes.append((_clear_of_faces(p_all[:4000].astype(np.float64), big).astype(np.float32), big, np.array([0])))  # every candidate collides
    t = dp.OBJECT_AUG.build(dict(type=kind, db_sampler=DB_SAMPLER), gt_database=db)
    batch = t(_batch(scenes))
    want_draws = _host_draws(state, db, scenes)
    for (r, g), (wr, wg) in zip(batch["db_sampled"], want_draws):
        assert np.array_equal(r, wr) and np.array_equal(g, wg)
    cyc = [int(np.sum(g == 2)) for _, g in batch["db_sampled"]]
    assert any(0 < c < 6 for c in cyc), cyc                         # the Cyclist sampler (3 objects) wrapped around
    want = _restated_paste(scenes, db, batch["db_sampled"], kind == "ObjectSample")
    acc = batch["db_accepted"].cpu().numpy().astype(bool)
    ks = np.cumsum([0] + [len(r) for r, _ in batch["db_sampled"]])
    got = _split(batch)
    for b, w in enumerate(want):
        assert np.array_equal(acc[ks[b]:ks[b + 1]], w["accepted"]), b
        assert np.array_equal(got[b][1], w["boxes"].astype(np.float32)), b
        assert np.array_equal(got[b][2], w["labels"]), b
        assert np.array_equal(got[b][0], w["points"].astype(np.float32)), b
    assert want[-1]["accepted"].size and not want[-1]["accepted"].any()
    assert sum(w["accepted"].sum() for w in want) > 10
    assert "count" not in batch and "gt_count" not in batch


def test_object_sample_reads_only_live_rows(cuda):
    """count / gt_count already set (PointsRangeFilter / ObjectRangeFilter before): only the live rows take part."""
    from uni3detr_amd import datapath as dp
    rng = np.random.default_rng(9)
    np.random.seed(9)
    db = _database(rng, 60)
    scenes = _scenes(rng, db, [(12000, 8), (9000, 5)])
    batch = _batch(scenes)
    batch = dp.PointsRangeFilter([5, -30, -3, 60, 30, 1])(batch)
    batch = dp.ObjectRangeFilter([5, -30, -3, 60, 30, 1])(batch)
    live = []
    cnt, gcnt = batch["count"].tolist(), batch["gt_count"].tolist()
    for b, (p, g, l) in enumerate(_split(batch)):
        live.append((p[:cnt[b]], g[:gcnt[b]], l[:gcnt[b]]))
    batch = dp.OBJECT_AUG.build(dict(type="ObjectSample", db_sampler=DB_SAMPLER), gt_database=db)(batch)
    want = _restated_paste(live, db, batch["db_sampled"], True)
    for b, (w, g) in enumerate(zip(want, _split(batch))):
        assert np.array_equal(g[0], w["points"].astype(np.float32)) and np.array_equal(g[1], w["boxes"].astype(np.float32)), b
        assert np.array_equal(g[2], w["labels"]), b


def test_object_noise_matches_restatement_and_keeps_points_in_their_box(cuda):
    from uni3detr_amd import datapath as dp
    rng = np.random.default_rng(4)
    np.random.seed(4)
    db = _database(rng, 60)
    scenes = _scenes(rng, db, [(20000, 15), (5000, 0), (12000, 20), (3000, 1)])
    batch = _batch(scenes)
    t = dp.OBJECT_AUG.build(dict(type="ObjectNoise", num_try=100, translation_std=[1.0, 1.0, 0.5], global_rot_range=[0.0, 0.0],
                                 rot_range=[-0.78539816, 0.78539816]))
    batch = t(batch)
    chosen = batch["object_noise_try"].cpu().numpy()
    go = batch["gt_off"].tolist()
    inside_checked = 0
    for b, ((p, g, _), (gp, gg, _)) in enumerate(zip(scenes, _split(batch))):
        loc, rot = batch["object_noise"]["loc"][b].astype(np.float64), batch["object_noise"]["rot"][b].astype(np.float64)
        wb, wp, wc = R.object_noise(g, p, loc, rot)
        assert np.array_equal(chosen[go[b]:go[b + 1]], wc), b
        np.testing.assert_allclose(gg, wb, rtol=1e-7, atol=1e-5)
        np.testing.assert_allclose(gp, wp, rtol=1e-7, atol=1e-5)
        # the local-frame invariant: every point of an original box is inside its noised box
        own = R.points_in_rbbox(p, g)
        for j in range(len(g)):
            m = own[:, j] & ~own[:, :j].any(1)
            assert R.points_in_rbbox(gp[m], gg[j:j + 1]).all(), (b, j)
            inside_checked += int(m.sum())
    assert inside_checked > 100 and (chosen >= 0).sum() > 10


def test_device_pipeline_opt_in_and_class_check(cuda):
    from uni3detr_amd import datapath as dp
    from uni3detr_amd.configs import pipelines as P
    for name in ("kitti_3classes", "kitti_car", "nuscenes"):
        pipe = dp.DevicePipeline(P.SHIPPED[name]["train_pipeline"])
        assert "ObjectSample" in pipe.skipped and ("ObjectNoise" in pipe.skipped or name == "nuscenes")
        assert not any(type(t).__name__ in ("ObjectSample", "ObjectNoise") for t in pipe.transforms)
    rng = np.random.default_rng(0)
    db = _database(rng, 20)
    cfg = _kitti_pipeline()
    with pytest.raises(ValueError):
        bad = copy.deepcopy(cfg)
        bad[2]["db_sampler"]["classes"] = ["Car", "Cyclist", "Pedestrian"]
        dp.DevicePipeline(bad, gt_database=db)
    with pytest.raises(NotImplementedError):
        dp.OBJECT_AUG.build(dict(type="ObjectSample", db_sampler=DB_SAMPLER, sample_2d=True), gt_database=db)
    pipe = dp.DevicePipeline(cfg, gt_database=db)
    assert "ObjectSample" not in pipe.skipped and "ObjectNoise" in pipe.skipped


def _kitti_pipeline():
    from uni3detr_amd.configs import pipelines as P
    cfg = copy.deepcopy(P.SHIPPED["kitti_3classes"]["train_pipeline"])
    for c in cfg:
        if c["type"] == "ObjectSample":
            c["db_sampler"] = dict(DB_SAMPLER, type="UnifiedDataBaseSampler")
        if c["type"] == "ObjectNoise":
            c.update(num_try=100, translation_std=[1.0, 1.0, 0.5], global_rot_range=[0.0, 0.0], rot_range=[-0.78539816, 0.78539816])
    return cfg


def test_kitti_train_pipeline_end_to_end_into_a_training_step(cuda):
    import projects.mmdet3d_plugin  # noqa: F401
    from uni3detr_amd import datapath as dp
    from uni3detr_amd.registry import build_model, to_config
    from uni3detr_amd.trainer import TrainStep
    rng = np.random.default_rng(21)
    np.random.seed(21)
    torch.manual_seed(0)
    db = _database(rng, 80)
    pipe = dp.DevicePipeline(_kitti_pipeline(), gt_database=db, object_noise=True)
    names = [type(t).__name__ for t in pipe.transforms]
    assert names[:2] == ["ObjectSample", "ObjectNoise"] and "ObjectSample" not in pipe.skipped and "ObjectNoise" not in pipe.skipped
    scenes = _scenes(rng, db, [(30000, 10), (25000, 4)])
    batch = pipe(_batch(scenes))
    pts, gts, labels = dp.unpack_batch(batch)
    assert [int(p.shape[0]) for p in pts] == [18000, 18000]
    assert all(int(g.tensor.shape[0]) == int(l.shape[0]) for g, l in zip(gts, labels))
    assert sum(int(l.shape[0]) for l in labels) > 14                # pasted objects survived the range filter
    shipped = os.path.join(os.path.dirname(__file__), "golden", "shipped_configs.txt")
    model = build_model(to_config(ast.literal_eval(open(shipped).read())["kitti_3classes"]["config"]["model"])).to(cuda).train()
    model.set_precision("bf16")
    ts = TrainStep(model, pts, gts, labels, graph=False, lr=1e-4)
    loss = float(ts.step())
    assert np.isfinite(loss) and loss > 0
