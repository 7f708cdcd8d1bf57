"""Dynamic voxelization in the captured inference step, on the GPU.

Kernels: u3d_scatter_mean_exact against the float64 mean under the header's bound (2^-23 |m| + 2^-shift max|v|), counts exactly, and
bit-identity across row permutations and calls, on a poisoned workspace and poisoned outputs; its argument checks; the spare rows of
u3d_voxelize_dynamic, alone and through DynamicSimpleVFE's static eval route.

Step: InferenceStep on the tiny ScanNet-large model (tests/dynvox_ref.py) under the seed discipline and the yardstick of
tests/test_infer_step_gpu.py - every compared forward starts from torch.manual_seed(SEED); a replay's class / box logits deviate from
set_precision('fp32') by at most 2 x what the eager folded forward does."""
import ctypes as C

import numpy as np
import pytest
import torch

import projects.mmdet3d_plugin  # noqa: F401
import dynvox_ref as ref
from test_varlen_gpu import _no_host_sync
from uni3detr_amd import native as nv
from uni3detr_amd.inference import InferenceModel, InferenceStep

pytestmark = pytest.mark.gpu
N, V = 4099, 37                 # rows: no multiple of 256 or 64, 17 blocks of 256 threads per feature count
SEED = 77


# ---- 1: the order-free mean -------------------------------------------------------------------------------------------------------
def _mean_case(name, nfeat):
    """-> (points f32 [n, nfeat], rank int32 [n], n_voxels); one row in eight has rank -1 wherever there are eight rows"""
    rng = np.random.default_rng(sum(map(ord, name)) + nfeat)
    n, v = N, V
    if name == "one_per_voxel":
        n = V
    elif name == "n1":
        n = 1
    elif name == "n0":
        n = 0
    pts = (rng.normal(0, 3, (n, nfeat))).astype(np.float32)
    rank = rng.integers(0, v, n).astype(np.int32)
    if name not in ("one_per_voxel", "n1", "n0"):
        rank[::8] = -1
    if name == "one_voxel":
        rank[rank >= 0] = 11
    elif name == "one_per_voxel":
        pts = (pts * 10.0 ** rng.uniform(-3, 3, pts.shape)).astype(np.float32)
        rank = rng.permutation(V).astype(np.int32)
    elif name == "empty_voxels":
        rank = np.where(rank >= 0, rank // 3 * 3, -1).astype(np.int32)                  # two voxels of three are never hit
    elif name == "zeros":
        pts[:] = 0
    elif name == "mixed":
        rows = np.flatnonzero(rank == 5)
        pts[rows] = (10.0 ** rng.uniform(-3, 3, (rows.size, nfeat)) * rng.choice([-1.0, 1.0], (rows.size, nfeat))).astype(np.float32)
        pts[rows[0]], pts[rows[1]] = 1e3, -1e-3
    elif name == "n1":
        rank[:] = 3
    return pts, rank, v


def _exact(cuda, pts, rank, v, poison=0xFF):
    """u3d_scatter_mean_exact through the C ABI on outputs and a workspace the caller did NOT zero -> (mean, counts) NumPy"""
    n, nfeat = pts.shape
    d_pts, d_rank = torch.from_numpy(pts).to(cuda), torch.from_numpy(rank).to(cuda)
    mean = torch.full((v, nfeat), float("nan"), device=cuda)
    counts = torch.full((v,), -7, dtype=torch.int32, device=cuda)
    wsb = int(nv.lib().u3d_scatter_mean_exact_workspace(v, nfeat))
    ws = torch.full((wsb // 8 + 1,), -1 if poison == 0xFF else 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=cuda)
    rc = nv.lib().u3d_scatter_mean_exact(nv._ptr(d_pts) if n else None, nv._ptr(d_rank) if n else None, n, nfeat, nv._ptr(mean), nv._ptr(counts), v,
                                         nv._ptr(ws), ws.numel() * 8, nv._stream())
    assert rc == 0, rc
    return mean.cpu().numpy(), counts.cpu().numpy()


@pytest.mark.parametrize("nfeat", [3, 4, 6])
@pytest.mark.parametrize("name", ["random", "one_voxel", "one_per_voxel", "empty_voxels", "zeros", "mixed", "n1", "n0"])
def test_exact_mean(cuda, name, nfeat):
    pts, rank, v = _mean_case(name, nfeat)
    n = pts.shape[0]
    got, cnt = _exact(cuda, pts, rank, v)
    m, big, want_cnt = ref.mean_f64(pts, rank, v)
    assert cnt.dtype == np.int32 and np.array_equal(cnt, want_cnt)
    shift = ref.shift_of(n)
    err, tol = np.abs(got.astype(np.float64) - m), ref.bound(m, big, shift)
    worst = float((err / np.where(tol > 0, tol, 1.0)).max()) if err.size else 0.0
    print(f"{name} F={nfeat}: n={n} shift={shift} largest error / bound = {worst:.3f}")
    assert shift == 40 and np.isfinite(got).all() and (err <= tol).all()
    assert not got[cnt == 0].any()                                                      # a row with no point: 0, count 0
    if name == "one_per_voxel":
        assert np.array_equal(got[rank].view(np.uint32), pts.view(np.uint32))           # a single point comes back with its bits
    if name == "one_voxel":
        assert cnt[11] == n - len(range(0, n, 8)) and cnt.sum() == cnt[11]
    if name == "empty_voxels":
        assert (cnt[1::3] == 0).all() and (cnt[2::3] == 0).all() and (cnt[::3] > 0).all()
    if name == "mixed":
        assert (big[5] == 1e3).all() and cnt[5] > 50
    if name == "n1":
        assert np.array_equal(got[3].view(np.uint32), pts[0].view(np.uint32)) and cnt.sum() == 1
    # the restatement computes the same three passes: the same bits
    want, _ = ref.scatter_mean_exact(pts, rank, v)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # any order of the rows, any call, another poison in the workspace: the same bytes
    again, cnt2 = _exact(cuda, pts, rank, v, poison=0x5A)
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32)) and np.array_equal(cnt2, cnt)
    for seed in (1, 2, 3):
        p = np.random.default_rng(seed).permutation(n)
        g, c = _exact(cuda, np.ascontiguousarray(pts[p]), np.ascontiguousarray(rank[p]), v)
        assert np.array_equal(g.view(np.uint32), got.view(np.uint32)) and np.array_equal(c, cnt), seed
    # the binding allocates its own outputs and workspace and returns the same
    if n:
        g, c = nv.scatter_mean_exact(torch.from_numpy(pts).to(cuda), torch.from_numpy(rank).to(cuda), v)
        assert np.array_equal(g.cpu().numpy().view(np.uint32), got.view(np.uint32)) and np.array_equal(c.cpu().numpy(), cnt)


def test_exact_mean_refuses_bad_arguments(cuda):
    """Both codes answer before any launch; every call here is well-formed apart from the one thing it names."""
    n, nfeat, v = 64, 3, 8
    pts, rank = torch.zeros((n, nfeat), device=cuda), torch.zeros((n,), dtype=torch.int32, device=cuda)
    mean, counts = torch.full((v, nfeat), 5.0, device=cuda), torch.full((v,), 5, dtype=torch.int32, device=cuda)
    wsb = int(nv.lib().u3d_scatter_mean_exact_workspace(v, nfeat))
    ws = torch.zeros(wsb // 8 + 1, dtype=torch.int64, device=cuda)
    p = nv._ptr
    ok = dict(points=p(pts), rank=p(rank), n_total=n, nfeat=nfeat, mean=p(mean), counts=p(counts), n_voxels=v, ws=p(ws), wsb=wsb)

    def call(**kw):
        a = dict(ok, **kw)
        return nv.lib().u3d_scatter_mean_exact(a["points"], a["rank"], a["n_total"], a["nfeat"], a["mean"], a["counts"], a["n_voxels"], a["ws"],
                                               a["wsb"], nv._stream())

    ARG, WS = -1, -4
    for name in ("points", "rank", "mean", "counts", "ws"):
        assert call(**{name: None}) == ARG, name
    assert call(n_total=-1) == ARG and call(nfeat=0) == ARG and call(nfeat=-3) == ARG and call(n_voxels=0) == ARG and call(n_voxels=-1) == ARG
    assert call(wsb=wsb - 1) == WS and call(wsb=0) == WS
    torch.cuda.synchronize()
    assert bool((mean == 5.0).all()) and bool((counts == 5).all())                      # nothing was launched
    assert call() == 0 and call(points=None, rank=None, n_total=0) == 0                 # no rows: no points needed
    assert not bool(mean.any()) and not bool(counts.any())
    assert "workspace" in nv.lib().u3d_strerror(WS).decode().lower()


# ---- 2: spare rows never become points -----------------------------------------------------------------------------------------------
VOX_B, VOX_P = 3, 300
VOX_SIZE, VOX_RANGE = [0.5, 0.5, 0.5], [-4.0, -4.0, 0.0, 4.0, 4.0, 2.0]                # a 4 x 16 x 16 grid: many points per voxel


def _vox_batch(cuda, sizes, seed):
    """B * P rows of which sum(sizes) are live (some out of range); the spare rows hold copies of in-range points"""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(VOX_RANGE[:3]), np.array(VOX_RANGE[3:])
    inside = lambda n: np.concatenate([rng.uniform(lo, hi - 1e-3, (n, 3)), rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)  # noqa: E731
    live = [inside(n) for n in sizes]
    for s in live:
        s[::7, :3] += 9.0                                                               # every seventh point out of range
    cat = np.concatenate(live) if sum(sizes) else np.zeros((0, 4), np.float32)
    pool = cat[np.all((cat[:, :3] >= lo) & (cat[:, :3] < hi), 1)] if sum(sizes) else inside(50)
    spare = pool[rng.integers(0, len(pool), VOX_B * VOX_P - len(cat))]
    full = torch.from_numpy(np.concatenate([cat, spare])).to(cuda)
    off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=cuda)
    return full, off, int(sum(sizes))


@pytest.mark.parametrize("sizes", [(120, 0, 300), (0, 17, 0), (0, 0, 0)])
def test_spare_rows_of_voxelize_dynamic(cuda, sizes):
    from uni3detr_amd.plugin.detector import DynamicSimpleVFE
    full, off, total = _vox_batch(cuda, sizes, seed=sum(sizes) + 1)
    assert full.shape[0] == VOX_B * VOX_P
    got = nv.voxelize_dynamic(full, off, VOX_B, VOX_SIZE, VOX_RANGE).cpu().numpy()
    assert (got[total:] == -1).all()                                                    # every spare row, all four columns
    if total == 0:
        return
    exact = nv.voxelize_dynamic(full[:total].contiguous(), off, VOX_B, VOX_SIZE, VOX_RANGE).cpu().numpy()
    assert got.tobytes() == ref.voxelize_dynamic_spare_rows(exact, VOX_B * VOX_P).tobytes()
    assert (exact[:, 0] >= 0).all() and (exact[:, 1] < 0).any() and (exact[:, 1] >= 0).any()      # in- and out-of-range live points
    # through DynamicSimpleVFE: the static eval route on the capacity-sized batch against the exact-size route on the live rows
    vfe = DynamicSimpleVFE(VOX_SIZE, VOX_RANGE).eval()
    vfe.exact_mean = True
    feats_e, coords_e = vfe(full[:total].contiguous(), torch.from_numpy(exact).to(cuda), batch_size=VOX_B)
    count = feats_e.shape[0]
    assert count == int(vfe.last_count_dev) > 0
    vfe.capacity, vfe.static_eval = 256 * ((count + 255) // 256 + 1), True
    feats_s, coords_s = vfe(full, torch.from_numpy(got).to(cuda), batch_size=VOX_B)
    assert feats_s.shape[0] == coords_s.shape[0] == vfe.capacity and int(vfe.last_count_dev) == count
    assert torch.equal(coords_s[:count], coords_e) and torch.equal(feats_s[:count].view(torch.int32), feats_e.view(torch.int32))
    assert bool((coords_s[count:] == -1).all()) and not bool(feats_s[count:].any())
    # the switch off again: a plain eval forward is exact-size whatever `capacity` says
    vfe.static_eval = False
    assert vfe(full[:total].contiguous(), torch.from_numpy(exact).to(cuda), batch_size=VOX_B)[0].shape[0] == count


# ---- 3: the step -------------------------------------------------------------------------------------------------------------------
B, P = 2, 12288
NAMES = ("boxes", "scores", "labels", "count", "off")


def _scenes(cuda, ids_sizes, pc_range):
    from uni3detr_amd.synth import room_scene
    out = [room_scene(i, n, pc_range=pc_range) for i, n in ids_sizes]
    return ([torch.from_numpy(o[0]).to(cuda) for o in out], [torch.from_numpy(o[1]).to(cuda) for o in out],
            [torch.from_numpy(o[2]).to(cuda) for o in out])


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _logits(outs):
    return outs["all_cls_scores"].double().clone(), outs["all_bbox_preds"].double().clone()


def _clone(det):
    return [getattr(det, n).clone() for n in NAMES]


def _same(x, y):
    return all(torch.equal(a, b) for a, b in zip(x, y))


def _run(step, pts, **kw):
    torch.manual_seed(SEED)
    return step.run(pts, **kw)


class _World:
    """Model, scenes, the fp32 reference logits and one captured step: built once, shared, left unchanged."""

    def __init__(self, cuda):
        from oracle.weights import seeded_tensor
        from uni3detr_amd.registry import build_model
        cfg = ref.tiny_scannet_large_cfg()
        self.pc_range = tuple(cfg["pts_voxel_layer"]["point_cloud_range"])
        model = build_model(cfg)
        model.load_state_dict({k: seeded_tensor(k, tuple(v.shape), 3) for k, v in model.state_dict().items()})
        self.model = model.to(cuda).eval()
        self.num_classes = int(model.pts_bbox_head.num_classes)
        self.a = _scenes(cuda, [(0, 9000), (1, 6500)], self.pc_range)[0]                 # B = 2, different point counts
        self.b = _scenes(cuda, [(5, 7000), (6, 8200)], self.pc_range)[0]
        self.model.set_precision("fp32")
        self.ref = self.fp32_logits(self.a)
        self.model.set_precision("bf16")
        self.inf = InferenceModel(self.model)
        torch.manual_seed(SEED)
        self.eager_logits = _logits(self.inf.head_outputs(self.a))
        self.eager = self.deviation(self.eager_logits)                                    # (cls, box) of the eager folded forward
        self.step = InferenceStep(self.inf, batch_size=B, point_capacity=P)
        self.counts, self.caps = self.step.capture(batches=[self.a, self.b], margin=1.25, warmup=3)

    def fp32_logits(self, pts):
        with torch.no_grad():
            feat, fps = self.model.extract_pts_feat(pts)
            torch.manual_seed(SEED)
            return _logits(self.model.pts_bbox_head(feat, None, fps))

    def deviation(self, logits, want=None):
        return tuple(_rel(x, r) for x, r in zip(logits, want or self.ref))


@pytest.fixture(scope="module")
def world(cuda):
    return _World(cuda)


def test_replay_against_eager(world):
    step, vfe = world.step, world.model.pts_voxel_encoder
    # the voxel list in front of the level capacities, sized like them and never above B * P rows
    assert len(world.caps) == len(world.counts) and world.caps[0] == step._vox_cap
    assert all(c % 256 == 0 and c >= n for c, n in zip(world.caps, world.counts)) and world.caps[0] <= B * P
    # every switch is back where a plain model.eval() forward expects it
    assert world.model.static_shapes is False and world.model.pts_middle_encoder.level_capacities is None
    assert (vfe.capacity, vfe.static_eval, vfe.exact_mean) == (None, False, False)
    det = _run(step, world.a)
    got = _logits(step.head_outs)
    dev = world.deviation(got)
    for what, g, e, x, y in zip(("cls", "box"), dev, world.eager, got, world.eager_logits):
        print(f"{what} logits: replay {g:.3e}  eager {e:.3e}  replay against eager {_rel(x, y):.3e}")
    print("replay logits bit-identical to the eager folded forward:", all(torch.equal(g, e) for g, e in zip(got, world.eager_logits)))
    for what, g, e in zip(("cls", "box"), dev, world.eager):
        assert g <= 2 * e, (what, g, e)
    # the replayed tail is the eager tail on the replay's own head outputs, bit for bit
    with torch.no_grad(), step.inf.scope():
        want = step.model.pts_bbox_head.get_bboxes_batched(step.head_outs, None)
    assert int(step.valid) == 1 and det.valid is step.valid
    for name in NAMES:
        assert torch.equal(getattr(det, name), getattr(want, name)), name
    assert int(det.count.sum()) > 0 and det.off.tolist() == np.concatenate([[0], np.cumsum(det.count.tolist())]).tolist()


def test_inputs_are_read(world):
    step = world.step
    a1, la1 = _clone(_run(step, world.a)), _logits(step.head_outs)
    b1, lb1 = _clone(_run(step, world.b)), _logits(step.head_outs)
    a2, la2 = _clone(_run(step, world.a)), _logits(step.head_outs)
    assert int(step.valid) == 1 and int(a1[3].sum()) > 0 and int(b1[3].sum()) > 0
    assert not _same(a1, b1)
    for what, x, y, e in zip(("cls", "box"), la1, lb1, world.eager):
        print(f"{what} logits: A vs B {_rel(y, x):.3e}  gate {2 * e:.3e}")
        assert _rel(y, x) > 10 * 2 * e
    assert _same(a1, a2) and all(torch.equal(x, y) for x, y in zip(la1, la2))           # A again: A's bits


def test_partial_batch(world):
    step = world.step
    det = _run(step, world.a[:1])
    cnt = det.count.tolist()
    assert int(step.valid) == 1 and cnt[0] > 0 and cnt[1] == 0
    assert not bool(det.boxes[1].any()) and not bool(det.scores[1].any()) and not bool(det.labels[1].any())
    assert det.off.tolist() == [0, cnt[0], cnt[0]]
    res = step.results(world.a[:1])
    assert len(res) == 1 and res[0]["boxes_3d"].shape[0] > 0 and not res[0]["boxes_3d"].is_cuda and step.fallbacks == 0


def test_stale_padding_never_becomes_points(world, cuda):
    """A large batch, then a small one: the rows the large one left behind the small one's scene_off[B] are spare capacity.  The small
    batch's result is that of a step that never saw the large one."""
    small = _scenes(cuda, [(7, 6000), (8, 6200)], world.pc_range)[0]
    step = world.step
    _run(step, world.a)
    assert int(step.pts["scene_off"][-1]) == 15500
    got, lg = _clone(_run(step, small)), _logits(step.head_outs)
    assert int(step.valid) == 1 and int(step.pts["scene_off"][-1]) == 12200
    assert bool(step.pts["cat"][12200:15500].any())                                     # the stale rows are really there
    fresh = InferenceStep(world.inf, batch_size=B, point_capacity=P)
    fresh.capture(batches=[world.a, world.b], margin=1.25, warmup=1)
    fresh._buf.pts["cat"].zero_()                                                       # as allocated: nothing behind the small batch
    want, lw = _clone(_run(fresh, small)), _logits(fresh.head_outs)
    assert int(fresh.valid) == 1 and int(want[3].sum()) > 0
    assert all(torch.equal(x, y) for x, y in zip(lg, lw)) and _same(got, want)


def test_voxel_list_overflow_is_gated_and_falls_back(world, cuda, monkeypatch):
    inf, enc = world.inf, world.model.pts_middle_encoder
    sparse = _scenes(cuda, [(7, 6000), (8, 6000)], world.pc_range)[0]
    dense = _scenes(cuda, [(9, 10000), (10, 10000)], world.pc_range)[0]
    step = InferenceStep(inf, batch_size=B, point_capacity=P)
    counts, caps = step.capture(batches=[sparse], margin=1.0, warmup=1)
    inf.extract_pts_feat(dense)
    voxels = int(enc.last_level_counts[0])
    print(f"voxel list: captured {counts[0]} -> capacity {caps[0]}; the dense batch has {voxels}")
    assert voxels > caps[0]                                                             # the list itself overflows
    det = _run(step, dense)
    assert int(step.valid) == 0 and det.count.tolist() == [0, 0] and det.off.tolist() == [0, 0, 0]
    assert not bool(det.boxes.any()) and not bool(det.scores.any()) and not bool(det.labels.any())
    # the fallback is one more eager forward: give the yardstick call the generator state the fallback started from
    seen, orig = [], inf.simple_test_batched
    monkeypatch.setattr(inf, "simple_test_batched", lambda *a, **k: seen.append(torch.cuda.get_rng_state(cuda)) or orig(*a, **k))
    res = step.results(dense)
    monkeypatch.undo()
    assert len(seen) == 1 and step.fallbacks == 1 and len(res) == B
    torch.cuda.set_rng_state(seen[0], cuda)
    want = inf.simple_test_batched(None, dense)
    assert sum(r["scores_3d"].shape[0] for r in want) > 0
    for r, w in zip(res, want):
        assert all(torch.equal(r[k], w[k]) for k in ("boxes_3d", "scores_3d", "labels_3d"))
    det = _run(step, sparse)                                                            # a following in-capacity batch is valid again
    assert int(step.valid) == 1 and int(det.count.sum()) > 0 and step.fallbacks == 1 and step.overflows() == 0


def test_packed_batch_runs_without_host_sync(world):
    from uni3detr_amd import datapath as dp
    step = world.step
    batch = dp.pack_batch(world.b)
    step.run(batch)                                                                     # (first use of the ingest: its one-time set-up)
    torch.cuda.synchronize()
    torch.manual_seed(SEED)
    with _no_host_sync():
        det = step.run(batch)
    torch.cuda.synchronize()
    assert int(step.valid) == 1 and step.pts["scene_off"].tolist() == [0, 7000, 15200]
    got = _clone(det)
    assert _same(got, _clone(_run(step, world.b))) and int(got[3].sum()) > 0             # the same points through the list path


def test_dataset_path_equals_the_per_batch_loop(world, cuda, tmp_path):
    """Five scenes, B = 2, from files: BatchFeeder + test_dataset + DetStore + add_store against results() + add() per batch."""
    from uni3detr_amd import datapath as dp
    from uni3detr_amd import evaluation as ev
    from uni3detr_amd import testing
    from uni3detr_amd.det_store import DetStore
    from uni3detr_amd.feeder import BatchFeeder
    from uni3detr_amd.synth import room_scene
    step, inf = world.step, world.inf
    samples, gts, labs = [], [], []
    for k, n in enumerate((6000, 7000, 8000, 9000, 6500)):
        p, g, l = room_scene(20 + k, n, pc_range=world.pc_range)
        path = str(tmp_path / f"scan{k}.bin")
        p.astype(np.float32).tofile(path)
        samples.append(dict(pts_filename=path))
        gts.append(torch.from_numpy(g).to(cuda))
        labs.append(torch.from_numpy(l % world.num_classes).to(cuda))
    cfg = [dict(type="LoadPointsFromFile", coord_type="DEPTH", shift_height=False, load_dim=4, use_dim=4),
           dict(type="PointsRangeFilter", point_cloud_range=list(world.pc_range)), dict(type="DefaultFormatBundle3D"), dict(type="Collect3D")]

    def feeder():
        return BatchFeeder(samples, range(5), dp.DevicePipeline(cfg, load=True), batch_size=B, device=cuda, drop_last=False)

    def scenes_of(batch):                   # the last batch holds one scene: run()'s list form pads and gates it
        return batch if batch["scene_off"].numel() == B + 1 else list(dp.unpack_batch(batch)[0])

    before = step.fallbacks
    a, k = ev.IndoorEvaluator(world.num_classes, device=cuda), 0
    with feeder() as f:
        for i, batch in enumerate(f):
            torch.manual_seed(SEED + i)
            res = step.results(scenes_of(batch))
            a.add(res, gts[k:k + len(res)], labs[k:k + len(res)])
            k += len(res)
    assert k == 5
    want = a.compute()
    store = DetStore(5, int(step.det.boxes.shape[1]), 7, cuda)
    with feeder() as f:
        testing.test_dataset(step, f, store, on_batch=lambda i: torch.manual_seed(SEED + i))
    b = ev.IndoorEvaluator(world.num_classes, device=cuda)
    b.add_store(store, gts, labs)
    got = b.compute()
    assert step.fallbacks == before and store.invalid_batches() == [] and len(store) == 5
    assert sum(r["scores_3d"].shape[0] for r in store.results()) > 0
    assert set(got) == set(want)
    for key in want:
        assert np.float64(got[key]).tobytes() == np.float64(want[key]).tobytes(), (key, got[key], want[key])


@pytest.mark.parametrize("option", ["sparse_levels", "dense_fp8"])
def test_composes_with_the_options(world, option):
    """Nothing in the dynamic route is specific to the folding options: the same gates on top of each."""
    inf = InferenceModel(world.model, **{option: True})
    if option == "dense_fp8":
        inf.calibrate([world.a])
    torch.manual_seed(SEED)
    eager = world.deviation(_logits(inf.head_outputs(world.a)))         # the reference path: the eager forward of the same options
    step = InferenceStep(inf, batch_size=B, point_capacity=P)
    step.capture(batches=[world.a], warmup=2)
    det = _run(step, world.a)
    got = world.deviation(_logits(step.head_outs))
    for what, g, e in zip(("cls", "box"), got, eager):
        print(f"{option} {what} logits: replay {g:.3e}  eager {e:.3e}")
    for what, g, e in zip(("cls", "box"), got, eager):
        assert g <= 2 * e, (option, what, g, e)
    with torch.no_grad(), inf.scope():
        want = step.model.pts_bbox_head.get_bboxes_batched(step.head_outs, None)
    assert int(step.valid) == 1 and int(det.count.sum()) > 0
    for name in NAMES:
        assert torch.equal(getattr(det, name), getattr(want, name)), name


def test_tta_replay(world, cuda):
    """views = 2 (plain + horizontal flip): one replay is valid and within 2 x the eager folded forward's deviation from fp32 over the
    same B * A views; its merged detections are those of inf.aug_test_batched on the same views."""
    from uni3detr_amd import datapath as dp
    A = 2
    inner = [dict(type="GlobalRotScaleTrans", rot_range=[0, 0], scale_ratio_range=[1.0, 1.0], translation_std=[0, 0, 0]),
             dict(type="RandomFlip3D"), dict(type="PointsRangeFilter", point_cloud_range=list(world.pc_range))]
    pipe = dp.DevicePipeline([dict(type="MultiScaleFlipAug3D", img_scale=(1333, 800), pts_scale_ratio=1, flip=True, pcd_horizontal_flip=True,
                                   transforms=inner)])
    batch = pipe(dp.pack_batch(list(world.b)))
    views = list(dp.unpack_batch(batch)[0])
    assert batch["tta_views"] == A and len(views) == B * A
    world.model.set_precision("fp32")
    want = world.fp32_logits(views)
    world.model.set_precision("bf16")
    torch.manual_seed(SEED)
    eager = world.deviation(_logits(world.inf.head_outputs(views)), want)
    step = InferenceStep(world.inf, batch_size=B, point_capacity=P, views=A)
    counts, caps = step.capture(batches=[batch], margin=1.25, warmup=1)
    assert len(caps) == len(counts) and caps[0] <= B * A * P
    det = _run(step, batch)
    assert int(step.valid) == 1 and tuple(step.view_det.boxes.shape[:1]) == (B * A,) and int(det.count.min()) > 0
    got = world.deviation(_logits(step.head_outs), want)
    for what, g, e in zip(("cls", "box"), got, eager):
        print(f"views=2 {what} logits: replay {g:.3e}  eager {e:.3e}")
    for what, g, e in zip(("cls", "box"), got, eager):
        assert g <= 2 * e, (what, g, e)
    torch.manual_seed(SEED)
    merged = world.inf.aug_test_batched(batch, on_device=True)
    print("views=2 merged detections bit-identical to inf.aug_test_batched:", _same(_clone(det)[:4], _clone(merged)[:4]))
