"""GPU: the capacity-mode training step (TrainStep(point_capacity=P)) and the device ingest that feeds it (u3d_batch_ingest,
uni3detr_amd/csrc/ingest.hip), all through the C ABI: the ingest against the NumPy restatement bit for bit, spare rows inert, the
capacity-mode step against the exact-size step, the captured step on batches of differing scene sizes loaded with
set_packed_batch, the nuScenes train pipeline end to end, no host traffic, overflow holds, set_batch with lists."""
import contextlib
import copy

import numpy as np
import pytest
import torch

import ingest_ref as R

pytestmark = pytest.mark.gpu

TOL = 2e-2          # relative loss tolerance of the replay-versus-eager check (tests/test_trainer_gpu.py)


# ---- fixtures built here ---------------------------------------------------------------------------------------------------------
def _model(kind, dev, sd=None):
    import projects.mmdet3d_plugin  # noqa: F401
    from uni3detr_amd.configs import variants
    from uni3detr_amd.registry import build_model
    torch.manual_seed(5)
    m = build_model(copy.deepcopy(getattr(variants, kind)))
    if sd is not None:
        m.load_state_dict(sd)
    for mod in m.modules():                       # dropout off: runs must be comparable
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if hasattr(mod, "attn_drop"):
            mod.attn_drop = 0.0
    return m.to(dev).train().set_precision("bf16")


def _scenes(kind, sizes, seed, dev, n_boxes=None):
    """room scenes in the configuration's range -> lists of points [n, 4 | 5], bottom-centre boxes [g, 7 | 9], labels int32"""
    from uni3detr_amd.configs import variants
    from uni3detr_amd.synth import room_scene
    cfg = getattr(variants, kind)
    rng_range = tuple(cfg["pts_voxel_layer"]["point_cloud_range"])
    nfeat, ncls = cfg["pts_middle_encoder"]["in_channels"], cfg["pts_bbox_head"]["num_classes"]
    rng = np.random.default_rng(seed)
    pts, boxes, labels = [], [], []
    for i, n in enumerate(sizes):
        g_n = 8 if n_boxes is None else n_boxes[i]
        p, g, l = room_scene(seed * 16 + i, n, n_boxes=g_n, pc_range=rng_range)
        if nfeat > 4:
            p = np.concatenate([p, rng.integers(0, 10, (p.shape[0], nfeat - 4)).astype(np.float32) * np.float32(0.05)], 1)
        g = g.copy()
        g[:, 2] -= g[:, 5] / 2
        if kind == "nuscenes":
            g = np.concatenate([g, rng.normal(0, 2, (g.shape[0], 2)).astype(np.float32)], 1)
        pts.append(torch.from_numpy(p).to(dev))
        boxes.append(torch.from_numpy(g).to(dev))
        labels.append(torch.from_numpy((l % ncls).astype(np.int32)).to(dev))
    return pts, boxes, labels


def _packed(kind, sizes, seed, dev, n_boxes=None, filtered=True):
    """a packed batch as a DevicePipeline returns it; filtered: through PointsRangeFilter, so it carries `count`"""
    from uni3detr_amd import datapath as dp
    from uni3detr_amd.configs import variants
    pts, boxes, labels = _scenes(kind, sizes, seed, dev, n_boxes)
    batch = dp.pack_batch(pts, boxes, "LiDAR", gt_labels_3d=labels)
    if filtered:
        batch = dp.PointsRangeFilter(list(getattr(variants, kind)["pts_voxel_layer"]["point_cloud_range"]))(batch)
    return batch


@contextlib.contextmanager
def _no_host_sync():
    """the installed torch honours the sync debug mode (a deliberate .item() raises under it, checked first)"""
    t = torch.ones(1, device="cuda")
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            t.item()
        yield
    finally:
        torch.cuda.set_sync_debug_mode(prev)


# ---- 3: the kernel against the restatement ---------------------------------------------------------------------------------------
SENT = -7.0


def _ingest_case(dev, F, dim, gd, sizes, counts, gsizes, gcounts, P, G, seed, flag0=0.0):
    from uni3detr_amd import native as nv
    rng = np.random.default_rng(seed)
    B = len(sizes)
    n, g = sum(sizes), sum(gsizes)
    pts = rng.normal(0, 20, (n + 5, F)).astype(np.float32)              # 5 rows of spare capacity behind scene_off[B]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    gt = rng.normal(0, 10, (g + 2, dim)).astype(np.float32)
    lab = rng.integers(0, 10, g + 2).astype(np.int32)
    goff = np.concatenate([[0], np.cumsum(gsizes)]).astype(np.int32)
    cnt = None if counts is None else np.asarray(counts, np.int32)
    gcnt = None if gcounts is None else np.asarray(gcounts, np.int32)
    guard = 16
    cat_r = np.full((B * P + guard, F), SENT, np.float32)
    gt_r, lab_r = np.full((B * G + guard, gd), SENT, np.float32), np.full(B * G + guard, int(SENT), np.int32)
    ref = R.batch_ingest(pts, off, cnt, P, cat_r, gt if g else None, lab, goff, gcnt, G, gt_r, lab_r, flag=flag0)
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)      # noqa: E731
    cat_d, gt_d, lab_d = t(np.full_like(cat_r, SENT)), t(np.full_like(gt_r, SENT)), t(np.full_like(lab_r, int(SENT)))
    dst_off, gt_off_out = torch.full((B + 1,), -1, dtype=torch.int32, device=dev), torch.full((B + 1,), -1, dtype=torch.int32, device=dev)
    flag, over = torch.full((1,), flag0, dtype=torch.float32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    nv.batch_ingest(t(pts), t(off), t(cnt), P, cat_d[:B * P], dst_off, flag, gt=t(gt), gt_labels=t(lab), gt_off=t(goff), gt_count=t(gcnt),
                    gt_cap=G, gt_out=gt_d[:B * G], labels_out=lab_d[:B * G], gt_off_out=gt_off_out, overflow=over)
    torch.cuda.synchronize()
    total, gtot = int(ref["dst_off"][-1]), int(ref["gt_off"][-1])
    assert torch.equal(dst_off.cpu(), torch.from_numpy(ref["dst_off"])) and torch.equal(gt_off_out.cpu(), torch.from_numpy(ref["gt_off"]))
    assert torch.equal(cat_d[:total].cpu(), torch.from_numpy(cat_r[:total]))
    assert torch.equal(gt_d[:gtot].cpu(), torch.from_numpy(gt_r[:gtot])) and torch.equal(lab_d[:gtot].cpu(), torch.from_numpy(lab_r[:gtot]))
    assert float(flag) == float(ref["flag"]) and over.tolist() == ref["overflow"].tolist()
    # nothing written behind the live rows, in particular nothing behind B * P / B * G: the guard rows keep their sentinel
    assert bool((cat_d[total:] == SENT).all()) and bool((gt_d[gtot:] == SENT).all()) and bool((lab_d[gtot:] == int(SENT)).all())
    return ref


@pytest.mark.parametrize("F", [4, 5])
@pytest.mark.parametrize("dim,gd", [(7, 7), (7, 9), (9, 9)])
def test_batch_ingest_matches_restatement(cuda, F, dim, gd):
    sizes, gsizes = [700, 0, 1300, 257, 64], [5, 0, 9, 1, 3]
    # whole segments, everything fits
    r = _ingest_case(cuda, F, dim, gd, sizes, None, gsizes, None, 1300, 9, 1)
    assert r["flag"] == 0.0
    # live prefixes (an empty one, a full one), still fits
    r = _ingest_case(cuda, F, dim, gd, sizes, [650, 0, 0, 257, 1], gsizes, [2, 0, 9, 0, 3], 700, 9, 2)
    assert r["flag"] == 0.0
    # point overflow only (scene 2 above P), the flag is added to
    r = _ingest_case(cuda, F, dim, gd, sizes, None, gsizes, [5, 0, 4, 1, 3], 1024, 5, 3, flag0=2.0)
    assert r["flag"] == 3.0 and r["overflow"].tolist() == [1, 0]
    # box overflow only, and both
    r = _ingest_case(cuda, F, dim, gd, sizes, [700, 0, 100, 257, 64], gsizes, None, 700, 4, 4)
    assert r["overflow"].tolist() == [0, 1]
    r = _ingest_case(cuda, F, dim, gd, sizes, None, gsizes, None, 256, 2, 5)
    assert r["overflow"].tolist() == [1, 1] and r["dst_off"].tolist() == [0, 256, 256, 512, 768, 832]
    # more scenes than one pass of the scan workgroup, and no boxes at all
    many = [int(v) for v in np.random.default_rng(9).integers(0, 40, 600)]
    _ingest_case(cuda, F, dim, gd, many, None, [1] * 600, None, 32, 1, 6)
    _ingest_case(cuda, F, dim, gd, sizes, None, [0] * 5, None, 1300, 3, 7)
    # an empty first, middle and last scene, on both sides
    _ingest_case(cuda, F, dim, gd, [0, 170, 0, 130, 0], None, [0, 3, 0, 2, 0], None, 170, 3, 8)


# ---- 4: spare rows are inert -----------------------------------------------------------------------------------------------------
def test_spare_rows_are_inert(cuda):
    """The same live data with the rows past scene_off[B] filled with NaN, 1e30 and zeros: bit-identical voxel coordinates, voxel
    means and FPS indices, and the same eager loss.  Voxel table and queries are the only consumers of the point buffer, so the
    losses see identical inputs; 1e-5 relative is two orders above float32 rounding of a reduction whose order may differ between
    launches, and far below what one stray voxel does to the BatchNorm statistics."""
    from uni3detr_amd import native as nv
    from uni3detr_amd.plugin.structures import Boxes3D
    sizes, P = [9000, 5000], 10240
    pts, boxes, labels = _scenes("kitti_3classes", sizes, 3, cuda)
    m = _model("kitti_3classes", cuda)
    B, n = len(sizes), sum(sizes)
    off = torch.tensor([0, sizes[0], n], dtype=torch.int32, device=cuda)
    gts = [Boxes3D(b) for b in boxes]
    got = []
    for fill in (float("nan"), 1e30, 0.0):
        cat = torch.full((B * P, 4), fill, dtype=torch.float32, device=cuda)
        cat[:n] = torch.cat(pts)
        d = dict(cat=cat, scene_off=off, lens=[P] * B)
        with torch.no_grad():
            coors, mean, voxel_off, _, _, _ = m.voxelize_batch(d)
            max_n = max(P, int(m.pts_voxel_layer.max_voxels[0]))
            _, idx = nv.fps_queries(cat, coors, off, voxel_off, B, max_n, m.num_fps)
        losses = m(return_loss=True, points=d, img_metas=None, gt_bboxes_3d=gts, gt_labels_3d=[l.long() for l in labels])
        loss = float(sum(v for k, v in losses.items() if "loss" in k))
        got.append((coors.clone(), mean.clone(), voxel_off.clone(), idx.clone(), loss))
    # and the exact-size buffer gives the same tables
    with torch.no_grad():
        e_coors, e_mean, e_off, _, _, _ = m.voxelize_batch(dict(cat=torch.cat(pts), scene_off=off, lens=sizes))
    assert int(got[0][2][-1]) > 1000 and np.isfinite(got[0][4])
    assert torch.equal(got[0][0], e_coors) and torch.equal(got[0][1], e_mean) and torch.equal(got[0][2], e_off)
    for c, mu, vo, idx, loss in got[1:]:
        assert torch.equal(c, got[0][0]) and torch.equal(mu, got[0][1]) and torch.equal(vo, got[0][2]) and torch.equal(idx, got[0][3])
        print("spare-row losses", loss, got[0][4])
        assert abs(loss - got[0][4]) <= 1e-5 * abs(got[0][4]), (loss, got[0][4])


# ---- 5: capacity-mode eager step == exact-size eager step ------------------------------------------------------------------------
@pytest.mark.parametrize("kind,sizes,P", [("kitti_3classes", [9000, 14000, 6000], 16384), ("nuscenes", [22000, 9000], 24576)])
def test_capacity_eager_step_equals_exact_eager_step(cuda, kind, sizes, P):
    """(the nuScenes case is the one with P > 20 480: the several-workgroup FPS in capacity mode)"""
    from uni3detr_amd.plugin.structures import Boxes3D
    from uni3detr_amd.trainer import TrainStep
    pts, boxes, labels = _scenes(kind, sizes, 11, cuda)
    gts, labs = [Boxes3D(b) for b in boxes], [l.long() for l in labels]
    m1 = _model(kind, cuda)
    sd = copy.deepcopy(m1.state_dict())
    exact = TrainStep(m1, pts, gts, labs, graph=False, lr=0.0, weight_decay=0.0)
    m2 = _model(kind, cuda, sd)
    cap = TrainStep(m2, pts, gts, labs, graph=False, lr=0.0, weight_decay=0.0, point_capacity=P)
    assert cap.pts["cat"].shape[0] == len(sizes) * P and cap.pts["lens"] == [P] * len(sizes)
    assert torch.equal(cap.pts["scene_off"], exact.pts["scene_off"])
    with torch.no_grad():
        ve, vc = m1.stage_voxelize(exact.pts), m2.stage_voxelize(cap.pts)
        fe, fc = m1.stage_fps(ve), m2.stage_fps(vc)
    assert torch.equal(ve["voxel_off"], vc["voxel_off"]) and torch.equal(ve["coors"], vc["coors"]) and torch.equal(ve["feats"], vc["feats"])
    assert torch.equal(fe, fc)
    le, lc = float(exact.step()), float(cap.step())
    print("exact / capacity loss", kind, le, lc)
    assert np.isfinite(le) and abs(lc - le) <= TOL * abs(le), (le, lc)
    assert cap.held_steps() == 0 and cap.ingest_overflows() == 0


# ---- 6 + 8: the headline -----------------------------------------------------------------------------------------------------------
def test_captured_capacity_step_trains_on_differing_scene_sizes(cuda):
    """One captured capacity-mode step; three packed batches whose scene sizes all differ (and differ from the capture batch's) go in
    with set_packed_batch - under the sync debug mode: no device-to-host copy - and each replayed loss equals the loss of a fresh eager
    exact-size step built from unpack_batch of the same batch.  No re-capture, no held step."""
    from uni3detr_amd import datapath as dp
    from uni3detr_amd.trainer import TrainStep
    kind, P = "nuscenes", 16384
    first = _packed(kind, [12000, 7000], 20, cuda)
    batches = [_packed(kind, s, 21 + i, cuda, n_boxes=g) for i, (s, g) in enumerate([([15000, 5000], [6, 11]), ([3000, 16000], [9, 2]),
                                                                                      ([9500, 11500], [12, 7])])]
    live = [b["count"].tolist() for b in [first] + batches]
    assert len({v for c in live for v in c}) == 8 and max(v for c in live for v in c) <= P          # all eight scene sizes differ
    m = _model(kind, cuda)
    sd = copy.deepcopy(m.state_dict())
    ts = TrainStep(m, *dp.unpack_batch(first), graph=True, lr=0.0, weight_decay=0.0, point_capacity=P)
    ts.capture(batches=batches + [first])
    ref = _model(kind, cuda, sd)
    for b in batches:
        with _no_host_sync():
            ts.set_packed_batch(b)
        l_replay = float(ts.step())
        eager = TrainStep(ref, *dp.unpack_batch(b), graph=False, lr=0.0, weight_decay=0.0)
        l_eager = float(eager.step())
        print("replay / eager loss", b["count"].tolist(), l_replay, l_eager)
        assert np.isfinite(l_eager) and abs(l_replay - l_eager) <= TOL * abs(l_eager), (l_replay, l_eager)
        assert torch.equal(ts.pts["scene_off"], eager.pts["scene_off"])
    assert ts.recaptures == 0 and ts.held_steps() == 0 and ts.ingest_overflows() == 0


# ---- 7: the shipped nuScenes train pipeline end to end -----------------------------------------------------------------------------
NUSC_CLASSES = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone"]
SWEEP_ENTRY = dict(type="LoadPointsFromMultiSweeps", sweeps_num=9, use_dim=[0, 1, 2, 3, 4], pad_empty_sweeps=True, remove_close=True)
TS_KEY = 1_533_151_603_547_000 / 1e6


def _write_sweeps(tmp_path, rng, sizes, prefix):
    out = []
    for j, n in enumerate(sizes):
        a = rng.uniform(-30, 30, (n, 5)).astype(np.float32)
        a[:, 2] = rng.uniform(-4, 2, n)
        path = str(tmp_path / f"{prefix}{j}.bin")
        a.tofile(path)
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)) * 0.05 + np.eye(3))
        out.append(dict(data_path=path, timestamp=1_533_151_603_000_000 - 50_000 * (j + 1), sensor2lidar_rotation=q * np.sign(np.linalg.det(q)),
                        sensor2lidar_translation=rng.normal(size=3) * 0.5))
    return out


def _nusc_pipeline():
    from uni3detr_amd.configs import pipelines as Pp
    cfg = copy.deepcopy(Pp.SHIPPED["nuscenes"]["train_pipeline"])
    for c in cfg:
        if c["type"] == "LoadPointsFromMultiSweeps":
            c.update(SWEEP_ENTRY)
        if c["type"] == "ObjectSample":
            c["db_sampler"] = dict(type="UnifiedDataBaseSampler", rate=1.0, classes=NUSC_CLASSES,
                                   sample_groups=dict(car=2, truck=3, bus=4, pedestrian=2, traffic_cone=2))
        if c["type"] == "ObjectNameFilter":
            c["classes"] = NUSC_CLASSES
    return cfg


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


def _nusc_batch(tmp_path, rng, tag, spec):
    """spec: per scene (key rows, sweeps, boxes) -> the packed host batch with its sweep records"""
    from uni3detr_amd import datapath as dp
    keys, infos, boxes, labs = [], [], [], []
    for b, (n, ns, g) in enumerate(spec):
        key = rng.uniform(-50, 50, (n, 5)).astype(np.float32)
        key[:, 2] = rng.uniform(-4, 2, n)
        sw = _write_sweeps(tmp_path, rng, [int(v) for v in rng.integers(200, 900, ns)], prefix=f"{tag}_{b}_")
        box = np.zeros((g, 9), np.float32)
        box[:, :2] = rng.uniform(-58, 58, (g, 2))
        box[:, 2] = -1.5
        box[:, 3:6] = rng.uniform(0.6, 4.5, (g, 3))
        box[:, 6] = rng.uniform(-np.pi, np.pi, g)
        box[:, 7:] = rng.normal(size=(g, 2))
        keys.append(torch.from_numpy(key).cuda()); infos.append(dict(timestamp=TS_KEY + b, sweeps=sw))
        boxes.append(torch.from_numpy(box).cuda()); labs.append(torch.from_numpy(rng.integers(-1, 10, g).astype(np.int32)).cuda())
    recs = [dp.read_sweeps(info, dict(SWEEP_ENTRY)) for info in infos]
    return dp.pack_batch(keys, boxes, "LiDAR", gt_labels_3d=labs, sweeps=recs)


def test_nuscenes_pipeline_feeds_the_captured_step(cuda, tmp_path):
    """sweep merge -> GT-paste -> rot / scale / flip -> range filters -> name filter -> PointShuffle on the device, then
    set_packed_batch -> captured step(), three batches of differing sizes: finite losses, the weights move, nothing is held."""
    from uni3detr_amd import datapath as dp
    from uni3detr_amd.trainer import TrainStep
    rng = np.random.default_rng(31)
    np.random.seed(31)
    torch.manual_seed(0)
    pipe = dp.DevicePipeline(_nusc_pipeline(), gt_database=_nusc_database(rng), sweeps=True, point_shuffle=True, name_filter=True)
    names = [type(t).__name__ for t in pipe.transforms]
    assert names[0] == "LoadPointsFromMultiSweeps" and "PointShuffle" in names and "ObjectNameFilter" in names and "PointSample" not in names
    specs = [[(3000, 9, 9), (1500, 0, 5)], [(2000, 12, 4), (2600, 3, 11)], [(3500, 5, 7), (1200, 9, 8)], [(1800, 0, 6), (3100, 7, 3)]]
    host = [_nusc_batch(tmp_path, rng, f"k{i}", s) for i, s in enumerate(specs)]
    with pytest.raises(ValueError):                                           # a batch whose sweeps were not merged is refused
        TrainStep.set_packed_batch(type("T", (), dict(point_capacity=1))(), host[0])
    outs = [pipe(b) for b in host]
    live = [o["count"].tolist() for o in outs]
    P = 20480
    assert len({v for c in live for v in c}) == 8 and 1000 < min(v for c in live for v in c) and max(v for c in live for v in c) <= P
    m = _model("nuscenes", cuda)
    ts = TrainStep(m, *dp.unpack_batch(outs[0]), graph=True, lr=1e-4, point_capacity=P, check_every=0)
    ts.capture(batches=outs)
    w = m.pts_bbox_head.cls_branches[0][0].weight
    for o in outs[1:]:
        w0 = w.detach().clone()
        with _no_host_sync():
            ts.set_packed_batch(o)
        loss = float(ts.step())
        print("pipeline batch", o["count"].tolist(), o["gt_count"].tolist(), loss)
        assert np.isfinite(loss) and loss > 0 and not torch.equal(w.detach(), w0)
    assert ts.held_steps() == 0 and ts.ingest_overflows() == 0 and ts.recaptures == 0


# ---- 9: overflow holds -------------------------------------------------------------------------------------------------------------
def test_ingest_overflow_holds_the_update_and_raises_at_the_check(cuda):
    from uni3detr_amd import datapath as dp
    from uni3detr_amd.trainer import TrainStep
    kind, P = "kitti_3classes", 8192
    ok1, ok2 = _packed(kind, [6000, 4000], 40, cuda), _packed(kind, [3000, 7000], 41, cuda)
    big = _packed(kind, [5000, 9000], 42, cuda)                               # second scene above P
    many = _packed(kind, [4500, 5500], 43, cuda, n_boxes=[3, 12])             # second scene above G = 10 boxes
    assert max(big["count"].tolist()) > P >= max(ok1["count"].tolist() + ok2["count"].tolist() + many["count"].tolist())
    m = _model(kind, cuda)
    ts = TrainStep(m, *dp.unpack_batch(ok1), graph=True, lr=1e-3, point_capacity=P, gt_capacity=10, check_every=3)
    ts.capture(batches=[ok1, ok2])
    state = lambda: (ts.flat_param.clone(), ts.exp_avg.clone(), ts.exp_avg_sq.clone())      # noqa: E731
    for bad, word in ((big, "point_capacity"), (many, "gt_capacity")):
        ts.set_packed_batch(ok1)
        before = state()
        ts.step()
        assert not torch.equal(ts.flat_param, before[0]) and ts.held_steps() == 0
        ts.set_packed_batch(bad)
        before = state()
        assert np.isfinite(float(ts.step()))
        assert all(torch.equal(a, b) for a, b in zip(state(), before))         # parameters and both moments untouched
        assert ts.held_steps() == 1 and ts.ingest_overflows() == 1
        ts.set_packed_batch(ok2)                                              # the next in-capacity batch trains normally
        ts.step()
        assert not torch.equal(ts.flat_param, before[0]) and ts.held_steps() == 1
        with pytest.raises(RuntimeError, match=word):                         # check_every = 3 steps later: the periodic check
            ts.step()
        assert ts.recaptures == 0 and ts.held_steps() == 0 and ts.ingest_overflows() == 0
    ts.step()                                                                 # and the step goes on after the report


# ---- 10: set_batch with lists in capacity mode -----------------------------------------------------------------------------------
def test_set_batch_with_lists_in_capacity_mode(cuda):
    from uni3detr_amd.plugin.structures import Boxes3D
    from uni3detr_amd.trainer import TrainStep
    kind, P = "kitti_3classes", 8192
    m = _model(kind, cuda)
    pts, boxes, labels = _scenes(kind, [5000, 3000], 50, cuda)
    with pytest.raises(ValueError):
        TrainStep(m, pts, [Boxes3D(b) for b in boxes], [l.long() for l in labels], graph=False, point_capacity=4096)
    ts = TrainStep(m, pts, [Boxes3D(b) for b in boxes], [l.long() for l in labels], graph=False, lr=1e-3, point_capacity=P, gt_capacity=10)
    l0 = float(ts.step())
    for sizes in ([8192, 100], [700, 6100]):
        p2, b2, l2 = _scenes(kind, sizes, 51 + sizes[0], cuda)
        ts.set_batch(p2, [Boxes3D(b) for b in b2], [l.long() for l in l2])
        before = ts.flat_param.clone()
        assert ts.pts["scene_off"].tolist() == [0, sizes[0], sum(sizes)]
        assert np.isfinite(float(ts.step())) and not torch.equal(ts.flat_param, before)
    assert np.isfinite(l0) and ts.held_steps() == 0
    keep = [ts.pts["cat"].clone(), ts.pts["scene_off"].clone(), ts.gts["gt"].clone(), ts.gts["labels"].clone(), ts.gts["gt_off"].clone()]
    p3, b3, l3 = _scenes(kind, [8193, 100], 60, cuda)
    with pytest.raises(ValueError):                                            # above P: before anything is written
        ts.set_batch(p3, [Boxes3D(b) for b in b3], [l.long() for l in l3])
    p4, b4, l4 = _scenes(kind, [100, 200], 61, cuda, n_boxes=[11, 2])
    with pytest.raises(ValueError):                                            # above gmax
        ts.set_batch(p4, [Boxes3D(b) for b in b4], [l.long() for l in l4])
    now = [ts.pts["cat"], ts.pts["scene_off"], ts.gts["gt"], ts.gts["labels"], ts.gts["gt_off"]]
    assert all(torch.equal(a, b) for a, b in zip(keep, now))
