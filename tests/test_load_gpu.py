"""LoadPointsFromFile and NormalizePointsColor on the device (uni3detr_amd/csrc/points_load.hip) against the NumPy restatement
(tests/load_ref.py), value-equal with equal NaN positions; the shipped SUN RGB-D and nuScenes train pipelines with the loader on the
device against the same pipelines fed host-loaded points; BatchFeeder against the synchronous loop, bit for bit; and the feeder's
batches through the captured training and inference steps."""
import copy

import numpy as np
import pytest
import torch

import load_ref as R

pytestmark = pytest.mark.gpu

SUN = dict(type="LoadPointsFromFile", coord_type="DEPTH", shift_height=True, load_dim=6, use_dim=[0, 1, 2])


def _raw(rng, n, load_dim=6):
    a = rng.uniform(-3, 3, (n, load_dim)).astype(np.float32)
    a[:, 2] = rng.normal(0.3, 0.9, n).astype(np.float32)
    if load_dim >= 6:
        a[:, -3:] = rng.integers(0, 256, (n, 3)).astype(np.float32)
    return a


def _records(tmp_path, raws, entry, tag="s"):
    from uni3detr_amd import datapath as dp
    recs = []
    for k, a in enumerate(raws):
        path = str(tmp_path / f"{tag}{k}.bin")
        a.tofile(path)
        recs.append(dp.read_points(path, entry))
    return recs


def _load(tmp_path, raws, entry, tag="s"):
    from uni3detr_amd import datapath as dp
    batch = dp.pack_batch(None, raw=_records(tmp_path, raws, entry, tag))
    assert batch["raw_points"].shape == (sum(len(a) for a in raws), entry["load_dim"]) and "points" not in batch
    off = batch["scene_off"].clone()
    out = dp.DevicePipeline([entry], load=True)(batch)
    assert torch.equal(out["scene_off"], off) and "raw_points" not in out and "load_table" not in out           # scene_off unchanged
    return out


def _check(out, raws, entry):
    e = {k: v for k, v in entry.items() if k != "type"}
    shift = e.get("shift_height", False)
    off = np.concatenate([[0], np.cumsum([len(a) for a in raws])])
    assert out["scene_off"].cpu().numpy().tolist() == off.tolist()
    pts = out["points"].cpu().numpy()
    fl = out["floor_height"].cpu().numpy() if shift else None
    assert ("floor_height" in out) == bool(shift)
    for b, a in enumerate(raws):
        want, wfl = R.load_points(a, e["use_dim"], shift)
        got = pts[off[b]:off[b + 1]]
        assert R.same(got, want), (b, len(a), np.argwhere(~(got == want))[:4])
        if shift:
            assert R.same(fl[b:b + 1], np.array([wfl], np.float32)), (b, fl[b], wfl)


def test_scene_sizes_in_one_batch(cuda, tmp_path):
    """1, 2, 3 rows; 101 rows (g = 0.99: the >= 0.5 branch); 257 and 1025 rows (one past a wave multiple / one past the select's
    workgroup); 5000 rows (i = 49)."""
    rng = np.random.default_rng(0)
    raws = [_raw(rng, n) for n in (1, 2, 3, 101, 257, 1025, 5000)]
    _check(_load(tmp_path, raws, SUN), raws, SUN)


def test_special_heights(cuda, tmp_path):
    rng = np.random.default_rng(1)
    equal = _raw(rng, 700)
    equal[:, 2] = np.float32(-1.25)
    zeros = _raw(rng, 300)
    zeros[:, 2] = np.where(rng.random(300) < 0.5, np.float32(0.0), np.float32(-0.0))
    zeros[:5, 2] = [1.0, -1.0, 2.0, -0.0, 0.0]
    around = _raw(rng, 5000)                       # i = 49: ranks 45 .. 49 share one value, rank 50 is the next distinct one
    order = np.argsort(around[:, 2], kind="stable")
    around[order[45:50], 2] = around[order[45], 2]
    across = _raw(rng, 5000)                       # ranks 47 .. 60 share one value: a == b
    order = np.argsort(across[:, 2], kind="stable")
    across[order[47:61], 2] = across[order[47], 2]
    coarse = _raw(rng, 4000)
    coarse[:, 2] = np.round(coarse[:, 2], 1)       # a handful of distinct heights
    neg = _raw(rng, 900)
    neg[:, 2] = -np.abs(neg[:, 2]) - 1
    wide = _raw(rng, 2000)
    wide[:, 2] = (rng.normal(0, 1, 2000) * 10.0 ** rng.integers(-30, 30, 2000)).astype(np.float32)     # every exponent byte
    raws = [equal, zeros, around, across, coarse, neg, wide]
    _check(_load(tmp_path, raws, SUN), raws, SUN)


def test_nan_scene_next_to_clean_scenes(cuda, tmp_path):
    rng = np.random.default_rng(2)
    raws = [_raw(rng, 400), _raw(rng, 1300), _raw(rng, 90)]
    raws[1][777, 2] = np.nan
    out = _load(tmp_path, raws, SUN)
    _check(out, raws, SUN)
    fl = out["floor_height"].cpu().numpy()
    pts = out["points"].cpu().numpy()
    assert np.isnan(fl[1]) and np.isfinite(fl[[0, 2]]).all()
    assert np.isnan(pts[400:1700, 3]).all() and np.isfinite(pts[:400]).all() and np.isfinite(pts[1700:]).all()
    assert np.isfinite(pts[400:1700, :3]).sum() == 1300 * 3 - 1


@pytest.mark.parametrize("name", ["scannet", "kitti_3classes", "nuscenes", "sunrgbd"])
@pytest.mark.parametrize("shift", [False, True])
def test_shipped_entries(cuda, tmp_path, name, shift):
    """load_dim 3 / 4 / 5 / 6 with the shipped use_dim settings, shift_height on and off"""
    from uni3detr_amd import datapath as dp
    entry = dict(dp.SHIPPED_LOAD_ENTRIES[name], shift_height=shift)
    rng = np.random.default_rng(entry["load_dim"])
    raws = [_raw(rng, n, entry["load_dim"]) for n in (513, 64, 1200)]
    out = _load(tmp_path, raws, entry)
    e = dp.OBJECT_AUG.build(entry)
    assert out["points"].shape[1] == e.feat == len(e.use_dim) + int(shift)
    _check(out, raws, dict(entry, use_dim=e.use_dim))


@pytest.mark.parametrize("shift,mean", [(False, None), (True, [127.5, 110.25, 96.0]), (False, [0.5, 1.5, 2.5])])
def test_use_color_and_normalize(cuda, tmp_path, shift, mean):
    from uni3detr_amd import datapath as dp
    entry = dict(type="LoadPointsFromFile", coord_type="DEPTH", load_dim=6, use_dim=[0, 1, 2, 3, 4, 5], shift_height=shift, use_color=True)
    rng = np.random.default_rng(8)
    raws = [_raw(rng, n) for n in (300, 1, 777)]
    batch = dp.pack_batch(None, raw=_records(tmp_path, raws, entry))
    pipe = dp.DevicePipeline([entry, dict(type="NormalizePointsColor", color_mean=mean)], load=True, normalize_color=True)
    out = pipe(batch)
    F = 6 + int(shift)
    assert out["color_dims"] == [F - 3, F - 2, F - 1]
    pts = out["points"].cpu().numpy()
    off = np.concatenate([[0], np.cumsum([len(a) for a in raws])])
    for b, a in enumerate(raws):
        want = R.normalize_color(R.load_points(a, entry["use_dim"], shift)[0], mean)
        assert R.same(pts[off[b]:off[b + 1]], want), b
    with pytest.raises(KeyError):                                           # without the colour attribute
        dp.NormalizePointsColor(mean)(_load(tmp_path, raws, SUN, tag="k"))


def test_empty_first_middle_and_last_scene(cuda):
    """the height column takes every row's scene from scene_off: scenes without rows in front, between and behind the others (the
    file reader refuses such a scene when the height is asked for, so this goes to the entry itself) - their floor is NaN"""
    from uni3detr_amd import datapath as dp
    from uni3detr_amd import native as nv
    from uni3detr_amd.eval_common import offsets
    rng = np.random.default_rng(12)
    raws = [_raw(rng, n) for n in (0, 170, 0, 130, 0)]                      # 300 rows: two workgroups of the gather
    tab = torch.from_numpy(dp.load_table([len(a) for a in raws])).to(cuda)
    pts, fl = nv.points_load(torch.from_numpy(np.concatenate(raws)).to(cuda), offsets([len(a) for a in raws], cuda), tab, [0, 1, 2], True)
    pts, fl = pts.cpu().numpy(), fl.cpu().numpy()
    assert pts.shape == (300, 4) and np.isnan(fl[[0, 2, 4]]).all()
    for b, lo in ((1, 0), (3, 170)):
        want, wfl = R.load_points(raws[b], [0, 1, 2], True)
        assert R.same(pts[lo:lo + len(want)], want) and R.same(fl[b:b + 1], np.array([wfl], np.float32))


def test_error_codes(cuda):
    from uni3detr_amd import native as nv
    import ctypes as C
    lib, p = nv.lib(), nv._ptr
    raw = torch.zeros((100, 6), device=cuda)
    off = torch.tensor([0, 40, 100], dtype=torch.int32, device=cuda)
    tab = torch.zeros((2, 2), dtype=torch.float64, device=cuda)
    out, fl = torch.zeros((100, 4), device=cuda), torch.zeros(2, device=cuda)
    need = int(lib.u3d_points_load_workspace(100, 1))
    assert need >= 400 and int(lib.u3d_points_load_workspace(100, 0)) == 0 and int(lib.u3d_points_load_workspace(-1, 1)) == -1
    ws = torch.zeros(need, dtype=torch.uint8, device=cuda)
    use = (C.c_int32 * 3)(0, 1, 2)

    def call(rows=100, ld=6, batch=2, n_use=3, shift=1, wsb=need, use=use, tab=tab, fl=fl):
        return lib.u3d_points_load(p(raw), rows, ld, p(off), batch, p(tab) if tab is not None else None, use, n_use, shift, p(ws), wsb,
                                   p(out), p(fl) if fl is not None else None, nv._stream())

    k = nv._K
    assert call() == k["U3D_OK"]
    assert call(wsb=need - 1) == k["U3D_ERR_WORKSPACE"] and call(wsb=0) == k["U3D_ERR_WORKSPACE"]
    assert call(shift=0, wsb=0) == k["U3D_OK"]
    for bad in (dict(ld=2), dict(ld=9), dict(batch=0), dict(rows=-1), dict(rows=1 << 31), dict(n_use=0), dict(n_use=2), dict(tab=None),
                dict(fl=None), dict(use=(C.c_int32 * 3)(0, 1, 6)), dict(use=(C.c_int32 * 3)(0, -1, 2))):
        assert call(**bad) == k["U3D_ERR_ARG"], bad
    assert lib.u3d_points_load(p(raw), 100, 6, p(off), 2, p(tab), (C.c_int32 * 8)(*range(8)), 8, 1, p(ws), need, p(out), p(fl),
                               nv._stream()) == k["U3D_ERR_ARG"]           # nine output columns
    pts = torch.zeros((10, 7), device=cuda)
    cn = lambda rows, feat, col0: lib.u3d_points_color_norm(p(pts), rows, feat, col0, 0.0, 0.0, 0.0, nv._stream())      # noqa: E731
    assert cn(10, 7, 4) == k["U3D_OK"] and cn(10, 7, 5) == k["U3D_ERR_ARG"] and cn(10, 2, 0) == k["U3D_ERR_ARG"]
    assert cn(-1, 7, 4) == k["U3D_ERR_ARG"] and cn(10, 7, -1) == k["U3D_ERR_ARG"] and cn(0, 7, 4) == k["U3D_OK"]
    with pytest.raises(ValueError):
        from uni3detr_amd import datapath as dp
        dp.OBJECT_AUG.build(dict(SUN, load_dim=5))(dict(raw_points=raw, scene_off=off))
    torch.cuda.synchronize()


# ---- the shipped pipelines end to end ------------------------------------------------------------------------------------------
def _boxes(rng, g, dim=7):
    b = np.zeros((g, dim), np.float32)
    b[:, :3] = rng.uniform(-2, 2, (g, 3))
    b[:, 3:6] = rng.uniform(0.3, 1.5, (g, 3))
    b[:, 6] = rng.uniform(-np.pi, np.pi, g)
    return b


def _sun_pipeline(num_points=None):
    from uni3detr_amd import datapath as dp
    from uni3detr_amd.configs import pipelines as P
    cfg = copy.deepcopy(P.SHIPPED["sunrgbd"]["train_pipeline"])
    for c in cfg:
        if c["type"] == "LoadPointsFromFile":
            c.update(dp.SHIPPED_LOAD_ENTRIES["sunrgbd"])
        if c["type"] == "PointSample" and num_points is not None:
            c["num_points"] = num_points
    return cfg


def _same_batch(a, b, keys=("points", "scene_off", "count", "gt_bboxes_3d", "gt_off", "gt_labels_3d", "gt_count")):
    for k in keys:
        assert (k in a) == (k in b), k
        if k in a:
            x, y = a[k], b[k]
            if k == "points":                               # exactly packed outputs may carry spare rows past scene_off[-1] / gt_off[-1]
                n = int(a["scene_off"][-1])
                x, y = x[:n], y[:n]
            if k in ("gt_bboxes_3d", "gt_labels_3d"):
                n = int(a["gt_off"][-1])
                x, y = x[:n].contiguous(), y[:n].contiguous()
            assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                                                              y.view(torch.int32) if y.dtype == torch.float32 else y), k


def test_sunrgbd_train_pipeline_equals_host_loaded(cuda, tmp_path):
    from uni3detr_amd import datapath as dp
    rng = np.random.default_rng(4)
    raws = [_raw(rng, n) for n in (5000, 1777, 12000)]
    gts = [_boxes(rng, g) for g in (4, 0, 9)]
    labs = [rng.integers(0, 10, len(g)).astype(np.int64) for g in gts]
    cfg = _sun_pipeline()
    on, off = dp.DevicePipeline(cfg, load=True), dp.DevicePipeline(cfg)
    assert "LoadPointsFromFile" in off.skipped and "LoadPointsFromFile" not in on.skipped
    np.random.seed(11)
    a = on(dp.pack_batch(None, gts, "Depth", gt_labels_3d=labs, raw=_records(tmp_path, raws, on.load_cfg)))
    host = [torch.from_numpy(R.load_points(r, [0, 1, 2], True)[0]).to(cuda) for r in raws]
    np.random.seed(11)
    b = off(dp.pack_batch(host, [torch.from_numpy(g).to(cuda) for g in gts], "Depth",
                          gt_labels_3d=[torch.from_numpy(l).to(cuda) for l in labs]))
    _same_batch(a, b)
    assert a["points"].shape == (3 * 100000, 4) and a["pcd_rotation_angle"].tolist() == b["pcd_rotation_angle"].tolist()


def test_nuscenes_train_pipeline_raw_and_sweeps_equals_host_loaded(cuda, tmp_path):
    import test_sweeps_gpu as S
    from uni3detr_amd import datapath as dp
    cfg = S._nusc_pipeline(True)
    for c in cfg:
        if c["type"] == "LoadPointsFromFile":
            c.update(dp.SHIPPED_LOAD_ENTRIES["nuscenes"])
    outs = []
    for device_load in (True, False):
        rng = np.random.default_rng(31)
        np.random.seed(31)
        db = S._nusc_database(rng)
        scenes = S._nusc_scenes(tmp_path, rng)
        pipe = dp.DevicePipeline(cfg, gt_database=db, sweeps=True, point_shuffle=True, name_filter=True, load=device_load)
        assert [type(t).__name__ for t in pipe.transforms][:2] == (["LoadPointsFromFile"] if device_load else []) + \
            ["LoadPointsFromMultiSweeps"] + ([] if device_load else ["ObjectSample"])
        sw = [dp.read_sweeps(info, dict(S.ENTRY)) for _, info, _, _ in scenes]
        if device_load:
            recs = _records(tmp_path, [k for k, _, _, _ in scenes], pipe.load_cfg, tag="key")
            batch = dp.pack_batch(None, [g for _, _, g, _ in scenes], "LiDAR", gt_labels_3d=[l for _, _, _, l in scenes], raw=recs, sweeps=sw)
            assert "points" not in batch and batch["sweeps"]["n_key"] == batch["raw_points"].shape[0]
        else:
            batch = dp.pack_batch([torch.from_numpy(k).cuda() for k, _, _, _ in scenes], [torch.from_numpy(g).cuda() for _, _, g, _ in scenes],
                                  "LiDAR", gt_labels_3d=[torch.from_numpy(l).cuda() for _, _, _, l in scenes], sweeps=sw)
        outs.append(pipe(batch))
    _same_batch(*outs)
    assert int(outs[0]["count"].min()) > 1000


# ---- the feeder ------------------------------------------------------------------------------------------------------------------
def _samples(tmp_path, rng, n, lo=200, hi=500):
    out = []
    for k in range(n):
        a = _raw(rng, int(rng.integers(lo, hi + 1)))
        path = str(tmp_path / f"feed{k}.bin")
        a.tofile(path)
        g = _boxes(rng, int(rng.integers(0, 6)))
        out.append(dict(pts_filename=path, gt_bboxes_3d=g, gt_labels_3d=rng.integers(0, 10, len(g)).astype(np.int64)))
    return out


def _sync_loop(samples, order, pipe, B, box_type="Depth"):
    from uni3detr_amd import datapath as dp
    out = []
    for i in range(0, len(order) - B + 1, B):
        idx = order[i:i + B]
        recs = [dp.read_points(samples[k], pipe.load_cfg) for k in idx]
        out.append(pipe(dp.pack_batch(None, [samples[k]["gt_bboxes_3d"] for k in idx], box_type,
                                      gt_labels_3d=[samples[k]["gt_labels_3d"] for k in idx], raw=recs)))
    return out


def _cpu(batch):
    return {k: v.cpu() for k, v in batch.items() if torch.is_tensor(v)}


def test_feeder_is_bit_identical_to_the_synchronous_loop(cuda, tmp_path):
    from uni3detr_amd import datapath as dp
    from uni3detr_amd.feeder import BatchFeeder
    rng = np.random.default_rng(6)
    samples = _samples(tmp_path, rng, 12)
    order = [int(v) for v in rng.permutation(12)] + [3]                     # 6 batches of 2 and one sample that drop_last drops
    cfg = _sun_pipeline(num_points=1024)
    np.random.seed(21)
    want = [_cpu(b) for b in _sync_loop(samples, order, dp.DevicePipeline(cfg, load=True), 2)]
    assert len(want) == 6
    for busy in (False, True):
        np.random.seed(21)
        got = []
        with BatchFeeder(samples, order, dp.DevicePipeline(cfg, load=True), batch_size=2, device=cuda) as f:
            for batch in f:
                if busy:                            # the consumer enqueues work of its own between the __next__ calls
                    x = torch.randn(1024, 1024, device=cuda)
                    for _ in range(20):
                        x = x @ x * 1e-3
                    keep = batch["points"] * 2.0
                    got.append((_cpu(batch), keep.cpu(), x))
                else:
                    got.append((_cpu(batch), None, None))
        assert len(got) == 6 and not f._reader.is_alive()
        for g, w in zip(got, want):
            assert set(g[0]) == set(w)
            for k in w:
                assert torch.equal(g[0][k], w[k]), (busy, k)
            if busy:
                assert torch.equal(g[1], w["points"] * 2.0)


def test_feeder_with_sweeps_is_bit_identical_to_the_synchronous_loop(cuda, tmp_path):
    """the sweep choice of every batch is drawn on the consumer's thread between the pipelines' draws, as the synchronous loop does"""
    import test_sweeps_gpu as S
    from uni3detr_amd import datapath as dp
    from uni3detr_amd.feeder import BatchFeeder
    rng = np.random.default_rng(13)
    cfg = [dict(dp.SHIPPED_LOAD_ENTRIES["nuscenes"]), dict(S.ENTRY), dict(type="UnifiedRotScaleTrans", rot_range=[-0.3925, 0.3925]),
           dict(type="PointsRangeFilter", point_cloud_range=[-54, -54, -5.0, 54, 54, 3.0])]
    samples = []
    for k, ns in enumerate([12, 0, 3, 15, 11, 10]):
        key = rng.uniform(-40, 40, (int(rng.integers(200, 500)), 5)).astype(np.float32)
        path = str(tmp_path / f"key{k}.bin")
        key.tofile(path)
        sw = S.write_sweeps(tmp_path, rng, [int(v) for v in rng.integers(50, 200, ns)], prefix=f"w{k}_")
        samples.append(dict(pts_filename=path, gt_bboxes_3d=None, gt_labels_3d=None, info=dict(timestamp=S.TS + k, sweeps=sw)))
    order = [0, 1, 2, 3, 4, 5, 3, 0]
    np.random.seed(2)
    pipe = dp.DevicePipeline(cfg, sweeps=True, load=True)
    want = []
    for i in range(0, len(order), 2):
        idx = order[i:i + 2]
        sw = [dp.read_sweeps(samples[k]["info"], pipe.sweeps_cfg) for k in idx]
        want.append(pipe(dp.pack_batch(None, None, "LiDAR", raw=[dp.read_points(samples[k], pipe.load_cfg) for k in idx], sweeps=sw)))
    np.random.seed(2)
    with BatchFeeder(samples, order, dp.DevicePipeline(cfg, sweeps=True, load=True), batch_size=2, device=cuda, box_type_3d="LiDAR") as f:
        got = list(f)
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert all(np.array_equal(a, b) for a, b in zip(g["sweep_choices"], w["sweep_choices"]))
        _same_batch(g, w)
        assert g["pcd_rotation_angle"].tolist() == w["pcd_rotation_angle"].tolist()
    assert any(len(c) == 9 and not np.array_equal(c, np.arange(9)) for g in got for c in g["sweep_choices"])     # real draws were made


# ---- captured steps --------------------------------------------------------------------------------------------------------------
def test_feeder_feeds_the_captured_training_step(cuda, tmp_path):
    """Three captured TrainStep(point_capacity=P) steps (lr = 0, so every loss depends on its batch alone) fed by the feeder and by
    the synchronous loop.  The ingested inputs are compared bit for bit.  The losses of two replays on identical inputs differ by
    the float-atomic reductions of the step only; the bound is the relative tolerance tests/test_trainer_gpu.py and
    tests/test_varlen_gpu.py use between a replay and its eager step (TOL)."""
    import test_varlen_gpu as V
    from uni3detr_amd import datapath as dp
    from uni3detr_amd.configs import variants
    from uni3detr_amd.feeder import BatchFeeder
    from uni3detr_amd.trainer import TrainStep
    kind, P = "kitti_3classes", 8192
    rng_range = list(getattr(variants, kind)["pts_voxel_layer"]["point_cloud_range"])
    cfg = [dict(dp.SHIPPED_LOAD_ENTRIES[kind]), dict(type="PointsRangeFilter", point_cloud_range=rng_range)]
    samples = []
    for i, sizes in enumerate(([6000, 4000], [3000, 7000], [5200, 4100], [2500, 6100])):
        pts, boxes, labels = V._scenes(kind, sizes, 70 + i, "cpu")
        for p, g, l in zip(pts, boxes, labels):
            path = str(tmp_path / f"train{len(samples)}.bin")
            p.numpy().tofile(path)
            samples.append(dict(pts_filename=path, gt_bboxes_3d=g.numpy(), gt_labels_3d=l.numpy()))
    order = list(range(8))
    pipe = dp.DevicePipeline(cfg, load=True)
    sync = _sync_loop(samples, order, pipe, 2, "LiDAR")
    m = V._model(kind, cuda)
    ts = TrainStep(m, *dp.unpack_batch(sync[0]), graph=True, lr=0.0, weight_decay=0.0, point_capacity=P)
    ts.capture(batches=sync)

    def run(batches):
        losses, inputs = [], []
        for b in batches:
            ts.set_packed_batch(b)
            n, g = int(ts.pts["scene_off"][-1]), int(ts.gts["gt_off"][-1])
            inputs.append((ts.pts["cat"][:n].clone(), ts.pts["scene_off"].clone(), ts.gts["gt"][:g].clone(), ts.gts["labels"][:g].clone()))
            torch.manual_seed(9)
            losses.append(float(ts.step()))
        return losses, inputs

    want, want_in = run(sync[1:])
    with BatchFeeder(samples, order[2:], dp.DevicePipeline(cfg, load=True), batch_size=2, device=cuda, box_type_3d="LiDAR") as f:
        got, got_in = run(f)
    assert len(got) == 3
    for a, b in zip(got_in, want_in):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    for l, w in zip(got, want):
        print("feeder / synchronous loss", l, w)
        assert np.isfinite(w) and abs(l - w) <= V.TOL * abs(w), (l, w)
    assert ts.recaptures == 0 and ts.held_steps() == 0 and ts.ingest_overflows() == 0


def test_feeder_feeds_the_captured_inference_step(cuda, tmp_path):
    """One InferenceStep.run(batch) on the feeder's batch against inf.simple_test_batched on the host-loaded scenes: the bound points
    are compared bit for bit, the replay returns the detections of the same scenes through the list path, and the replay's head
    logits deviate from the fp32 reference by at most twice the eager folded forward's deviation (the gate of
    tests/test_infer_step_gpu.py)."""
    import test_infer_step_gpu as I
    from uni3detr_amd import datapath as dp
    from uni3detr_amd.feeder import BatchFeeder
    from uni3detr_amd.synth import room_scene
    from oracle.weights import seeded_tensor
    from uni3detr_amd.inference import InferenceModel, InferenceStep
    from uni3detr_amd.registry import build_model
    model = build_model(I.tiny_cfg())
    model.load_state_dict({k: seeded_tensor(k, tuple(v.shape), 3) for k, v in model.state_dict().items()})
    model = model.to(cuda).eval()
    rng = np.random.default_rng(3)
    raws, samples = [], []
    for k, (i, n) in enumerate([(0, 9000), (1, 6500)]):                     # the scenes of world.a as six-column files
        xyz = room_scene(i, n)[0][:, :3]
        raws.append(np.concatenate([xyz, rng.integers(0, 256, (n, 3)).astype(np.float32)], 1))
        path = str(tmp_path / f"inf{k}.bin")
        raws[-1].tofile(path)
        samples.append(dict(pts_filename=path, gt_bboxes_3d=None, gt_labels_3d=None))
    host = [torch.from_numpy(R.load_points(r, [0, 1, 2], True)[0]).to(cuda) for r in raws]
    pipe = dp.DevicePipeline([SUN], load=True)
    with BatchFeeder(samples, [0, 1], pipe, batch_size=2, device=cuda) as f:
        batch = next(f)
    model.set_precision("fp32")
    with torch.no_grad():
        feat, fps = model.extract_pts_feat(host)
        torch.manual_seed(I.SEED)
        fp32 = I._logits(model.pts_bbox_head(feat, None, fps))
    model.set_precision("bf16")
    inf = InferenceModel(model)
    eager = tuple(I._rel(x, r) for x, r in zip(I._logits(I._eager(inf, host)), fp32))
    step = InferenceStep(inf, batch_size=2, point_capacity=I.P)
    step.capture(batches=[host], margin=1.25, warmup=1)
    det = I._run(step, batch)
    assert int(step.valid) == 1 and int(det.count.sum()) > 0
    n = int(step.pts["scene_off"][-1])
    assert step.pts["scene_off"].tolist() == [0, 9000, 15500] and torch.equal(step.pts["cat"][:n], torch.cat(host))
    replay = tuple(I._rel(x, r) for x, r in zip(I._logits(step.head_outs), fp32))
    for what, g, e in zip(("cls", "box"), replay, eager):
        print(f"feeder batch {what} logits: replay {g:.3e}  eager {e:.3e}")
        assert g <= 2 * e, (what, g, e)
    torch.manual_seed(I.SEED)
    res = inf.simple_test_batched(None, host)
    got = step.results(batch)
    assert len(got) == len(res) == 2 and step.fallbacks == 0
    assert all(set(g) == set(r) and g["boxes_3d"].shape[1:] == r["boxes_3d"].shape[1:] for g, r in zip(got, res))
