"""Host side of the on-device LoadPointsFromFile (datapath.read_points, datapath.load_table) against the restatement
(tests/load_ref.py), the declared floor rule against np.percentile, the argument and empty-file errors, the DevicePipeline opt-ins,
and BatchFeeder's ordering, error propagation and shutdown with a fake pack / pipeline (no GPU)."""
import threading
import time

import numpy as np
import pytest

import load_ref as R

SUN_ENTRY = dict(type="LoadPointsFromFile", coord_type="DEPTH", shift_height=True, load_dim=6, use_dim=[0, 1, 2])
SIZES = [1, 2, 3, 100, 101, 102, 203, 5000]


def _scan(rng, n, load_dim=6):
    a = rng.uniform(-3, 3, (n, load_dim)).astype(np.float32)
    a[:, 2] = rng.normal(0.4, 0.8, n).astype(np.float32)
    return a


@pytest.mark.parametrize("ext", [".bin", ".npy"])
def test_read_points_equals_restatement(tmp_path, ext):
    from uni3detr_amd import datapath as dp
    a = _scan(np.random.default_rng(1), 777)
    path = str(tmp_path / ("scan" + ext))
    if ext == ".npy":
        np.save(path, a)
    else:
        a.tofile(path)
    for arg in (path, tmp_path / ("scan" + ext), dict(pts_filename=path)):
        rec = dp.read_points(arg, SUN_ENTRY)
        assert rec["load_dim"] == 6 and rec["raw"].dtype == np.float32 and rec["raw"].flags.c_contiguous
        assert np.array_equal(rec["raw"], R.read_file(path, 6)) and np.array_equal(rec["raw"], a)
    assert set(rec) == {"raw", "load_dim"}                                  # it does nothing else


def test_index_and_gamma_table_equals_numpys():
    from uni3detr_amd import datapath as dp
    tab = dp.load_table(SIZES)
    assert tab.dtype == np.float64 and tab.shape == (len(SIZES), 2)
    for row, n in zip(tab, SIZES):
        i, g = R.index_and_gamma(n)
        assert row[0] == i and row[1] == g, (n, row, i, g)
    assert tab[0].tolist() == [0.0, 0.0] and tab[4, 0] == 0 and tab[4, 1] >= 0.5 and tab[7, 0] == 49       # 101 rows: the >= 0.5 branch


@pytest.mark.parametrize("n", SIZES)
def test_float64_rule_reproduces_np_percentile_exactly(n):
    rng = np.random.default_rng(n)
    for trial in range(8):
        z = rng.normal(0.4, 0.8, n).astype(np.float32)
        if trial == 7:
            z = np.round(z, 1)                                             # heavy duplicates
        z64 = z.astype(np.float64)
        assert R.floor_by_rule(z) == np.percentile(z64, 0.99)
        assert np.float32(R.floor_by_rule(z)) == R.floor_height(z)


@pytest.mark.parametrize("n", SIZES)
def test_float32_input_percentile_is_within_one_ulp(n):
    """NumPy versions differ in how they interpolate float32 input (upstream ran one of them): the distance is reported, not hidden."""
    rng = np.random.default_rng(100 + n)
    worst = 0.0
    for _ in range(8):
        z = rng.normal(0.4, 0.8, n).astype(np.float32)
        ref = R.floor_height(z)
        got = np.float32(np.percentile(z, 0.99))
        ulp = abs(float(got) - float(ref)) / float(np.spacing(np.abs(ref)))
        worst = max(worst, ulp)
    print(f"float32-input np.percentile (numpy {np.__version__}) vs the float64 rule, n = {n}: {worst} ulp")
    assert worst <= 1.0


def test_argument_errors_and_empty_file(tmp_path):
    from uni3detr_amd import datapath as dp
    L = dp.LoadPointsFromFile
    with pytest.raises(NotImplementedError):
        L("DEPTH", file_client_args=dict(backend="petrel"))
    with pytest.raises(NotImplementedError):
        dp.read_points("x.bin", dict(SUN_ENTRY, file_client_args=dict(backend="disk", path_mapping={})))
    for bad in (dict(load_dim=2), dict(load_dim=9, use_dim=3), dict(load_dim=8, use_dim=8, shift_height=True)):
        with pytest.raises(NotImplementedError):
            L("LIDAR", **bad)
    with pytest.raises(ValueError):
        L("LIDAR", load_dim=4, use_dim=[0, 1, 4])
    with pytest.raises(ValueError):
        L("LIDAR", load_dim=4, use_dim=[0, 1], shift_height=True)
    with pytest.raises(ValueError):
        L("DEPTH", load_dim=6, use_dim=[0, 1, 2], use_color=True)
    with pytest.raises(ValueError):
        L("SPHERE")
    e = L("LIDAR", load_dim=5, use_dim=4)
    assert e.use_dim == [0, 1, 2, 3] and e.feat == 4 and L("DEPTH", shift_height=True).feat == 4
    with pytest.raises(ValueError):
        dp.NormalizePointsColor(color_mean=[1, 2])
    with pytest.raises(KeyError):
        dp.NormalizePointsColor()(dict(points=None))                        # no colour attribute
    with pytest.raises(KeyError):
        L("DEPTH")(dict(points=None))                                       # no raw rows
    empty = str(tmp_path / "empty.bin")
    np.zeros((0, 6), np.float32).tofile(empty)
    with pytest.raises(ValueError, match="no point"):
        dp.read_points(empty, SUN_ENTRY)
    assert dp.read_points(empty, dict(SUN_ENTRY, shift_height=False))["raw"].shape == (0, 6)
    odd = str(tmp_path / "odd.bin")
    np.zeros(13, np.float32).tofile(odd)
    with pytest.raises(ValueError):                                         # not a multiple of load_dim
        dp.read_points(odd, SUN_ENTRY)
    with pytest.raises(ValueError):
        dp.pack_batch([], raw=[dict(raw=np.zeros((1, 6), np.float32), load_dim=6)])


def test_device_pipeline_opt_ins():
    from uni3detr_amd import datapath as dp
    from uni3detr_amd.configs import pipelines as P
    cfg = [dict(c, **dp.SHIPPED_LOAD_ENTRIES["sunrgbd"]) if c["type"] == "LoadPointsFromFile" else c
           for c in P.SHIPPED["sunrgbd"]["train_pipeline"]]
    assert dp.SHIPPED_LOAD_ENTRIES["sunrgbd"] == SUN_ENTRY and set(dp.SHIPPED_LOAD_ENTRIES) == set(P.SHIPPED)
    off = dp.DevicePipeline(cfg)
    assert "LoadPointsFromFile" in off.skipped and off.load_cfg is None
    on = dp.DevicePipeline(cfg, load=True)
    assert type(on.transforms[0]).__name__ == "LoadPointsFromFile" and "LoadPointsFromFile" not in on.skipped
    assert on.load_cfg["type"] == "LoadPointsFromFile" and on.transforms[0].shift_height and on.transforms[0].feat == 4
    assert [type(t).__name__ for t in on.transforms[1:]] == [type(t).__name__ for t in off.transforms]
    col = dp.DevicePipeline([dict(type="LoadPointsFromFile", coord_type="DEPTH", load_dim=6, use_dim=6, use_color=True),
                             dict(type="NormalizePointsColor", color_mean=None)], load=True, normalize_color=True)
    assert [type(t).__name__ for t in col.transforms] == ["LoadPointsFromFile", "NormalizePointsColor"] and not col.skipped


# ---- the feeder without a GPU: a fake pack and a fake pipeline -----------------------------------------------------------------
def _files(tmp_path, n, rows=50):
    rng = np.random.default_rng(7)
    out = []
    for k in range(n):
        path = str(tmp_path / f"f{k}.bin")
        a = _scan(rng, rows + k)
        a[:, 0] = k
        a.tofile(path)
        out.append(dict(pts_filename=path, gt_bboxes_3d=np.full((k % 3, 7), k, np.float32), gt_labels_3d=np.full(k % 3, k, np.int64)))
    return out


def _fake_pack(points, gt, box_type_3d, gt_labels_3d=None, raw=None, device=None, **kw):
    assert points is None and threading.current_thread() is threading.main_thread()
    return dict(ids=[int(r["raw"][0, 0]) for r in raw], rows=[r["raw"].shape[0] for r in raw], gt=gt, labels=gt_labels_3d, draws=[])


class _FakePipe:
    load_cfg = dict(SUN_ENTRY)

    def __call__(self, batch):
        assert threading.current_thread() is threading.main_thread()
        batch["draws"].append(float(np.random.rand()))
        return batch


@pytest.mark.parametrize("drop_last", [True, False])
def test_feeder_preserves_order_and_draw_order(tmp_path, drop_last):
    from uni3detr_amd.feeder import BatchFeeder
    samples = _files(tmp_path, 9)
    order = [4, 0, 7, 7, 2, 8, 1, 3, 5, 6, 0]
    np.random.seed(5)
    with BatchFeeder(samples, order, _FakePipe(), batch_size=2, device="cpu", pack=_fake_pack, drop_last=drop_last) as f:
        got = list(f)
    np.random.seed(5)
    want_draws = [float(np.random.rand()) for _ in range(6)]
    want = [order[i:i + 2] for i in range(0, len(order), 2)]
    if drop_last:
        want = want[:-1]
    assert [b["ids"] for b in got] == want
    assert [b["rows"] for b in got] == [[50 + k for k in w] for w in want]
    assert [b["draws"][0] for b in got] == want_draws[:len(want)]
    assert all(len(b["gt"]) == len(b["ids"]) and b["gt"][0].shape == (b["ids"][0] % 3, 7) for b in got)
    assert not f._reader.is_alive()


def test_feeder_reraises_a_reader_exception_on_the_consumer(tmp_path):
    from uni3detr_amd.feeder import BatchFeeder
    samples = _files(tmp_path, 4)
    samples.append(dict(pts_filename=str(tmp_path / "missing.bin"), gt_bboxes_3d=None, gt_labels_3d=None))
    short = str(tmp_path / "short.bin")
    np.zeros(7, np.float32).tofile(short)
    samples.append(dict(pts_filename=short, gt_bboxes_3d=None, gt_labels_3d=None))
    for bad, exc in ((4, FileNotFoundError), (5, ValueError)):
        f = BatchFeeder(samples, [0, 1, 2, bad, 3, 0], _FakePipe(), batch_size=2, device="cpu", pack=_fake_pack)
        assert next(f)["ids"] == [0, 1]
        with pytest.raises(exc):
            next(f)
        f._reader.join(timeout=5.0)
        assert not f._reader.is_alive()
        with pytest.raises(StopIteration):
            next(f)


def test_feeder_close_joins_the_reader(tmp_path):
    from uni3detr_amd.feeder import BatchFeeder
    samples = _files(tmp_path, 6)
    f = BatchFeeder(samples, iter(range(6)), _FakePipe(), batch_size=2, device="cpu", pack=_fake_pack)
    assert next(f)["ids"] == [0, 1] and f._reader.is_alive()
    t0 = time.monotonic()
    f.close()
    f._reader.join(timeout=5.0)
    assert not f._reader.is_alive() and time.monotonic() - t0 < 5.0
    f.close()                                                               # idempotent
    with pytest.raises(ValueError):
        BatchFeeder(samples, [0], type("P", (), {"__call__": lambda s, b: b})(), batch_size=1, device="cpu", pack=_fake_pack)
    with pytest.raises(ValueError):
        BatchFeeder(samples, [0], _FakePipe(), batch_size=1, depth=1, device="cpu", pack=_fake_pack)
