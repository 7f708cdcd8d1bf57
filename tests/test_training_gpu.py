"""training.fit, the step log inside the captured step, resume, the validation hook, a held batch and the command line, end to end on
the device.  The shape: the tiny model of tests/test_bn_fold_cpu.py in bf16, 6 room scenes of 2 000 to 3 000 points as .bin files in
the SUN RGB-D indoor layout, B = 2, 2 epochs of 3 iterations, a captured step with point_capacity from plan_point_capacity.  Two
captured steps are built once per module (identical weights); every test starts them from the state they had after the capture."""
import copy
import json
import os
import pickle

import numpy as np
import pytest
import torch

from test_bn_fold_cpu import tiny_cfg
from test_varlen_gpu import _no_host_sync

pytestmark = pytest.mark.gpu

RANGE = [-3.2, -0.2, -2.0, 3.2, 6.2, 0.56]
LOAD = dict(type="LoadPointsFromFile", coord_type="DEPTH", shift_height=True, load_dim=6, use_dim=[0, 1, 2])
TRAIN_PIPELINE = [LOAD, dict(type="LoadAnnotations3D"), dict(type="RandomFlip3D", sync_2d=False, flip_ratio_bev_horizontal=0.5),
                  dict(type="GlobalRotScaleTrans", rot_range=[-0.2, 0.2], scale_ratio_range=[0.95, 1.05], shift_height=True),
                  dict(type="PointsRangeFilter", point_cloud_range=RANGE), dict(type="DefaultFormatBundle3D"), dict(type="Collect3D")]
TEST_PIPELINE = [LOAD, dict(type="PointsRangeFilter", point_cloud_range=RANGE), dict(type="DefaultFormatBundle3D"), dict(type="Collect3D")]
SIZES = (2000, 2300, 2500, 2700, 2900, 3000)
BIG = 6000
B, EPOCHS, IPE = 2, 2, 3


def _write_dataset(root):
    """6 scenes + one above any capacity planned from them -> (ann_file of the 6, the path of the big scene's .bin)"""
    from uni3detr_amd.datasets import SUNRGBD_CLASSES
    from uni3detr_amd.synth import room_scene
    rng = np.random.default_rng(3)
    os.makedirs(os.path.join(root, "points"), exist_ok=True)
    infos = []
    for k, n in enumerate(SIZES + (BIG,)):
        p, g, l = room_scene(40 + k, n, n_boxes=4 + k % 3)
        path = os.path.join("points", f"{k:06d}.bin")
        np.concatenate([p[:, :3], rng.integers(0, 256, (n, 3)).astype(np.float32)], 1).tofile(os.path.join(root, path))
        l = (l % 10).astype(np.int64)
        infos.append(dict(point_cloud=dict(num_features=6, lidar_idx=k), pts_path=path,
                          annos=dict(gt_num=len(l), gt_boxes_upright_depth=g.astype(np.float32), name=np.array([SUNRGBD_CLASSES[c] for c in l]),
                                     **{"class": l})))
    ann = os.path.join(root, "sunrgbd_infos_train.pkl")
    with open(ann, "wb") as f:
        pickle.dump(infos[:len(SIZES)], f)
    big = os.path.join(root, "big_infos.pkl")
    with open(big, "wb") as f:
        pickle.dump(infos, f)
    return ann, big


def _model(dev, sd=None):
    import projects.mmdet3d_plugin  # noqa: F401
    from uni3detr_amd.registry import build_model
    torch.manual_seed(5)
    m = build_model(tiny_cfg())
    if sd is not None:
        m.load_state_dict(sd)
    for mod in m.modules():                       # dropout off: runs must be comparable
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if hasattr(mod, "attn_drop"):
            mod.attn_drop = 0.0
    return m.to(dev).train().set_precision("bf16")


class _Run:
    """one captured step over the synthetic set, with what fit needs around it"""

    def __init__(self, dev, samples, sd=None):
        from uni3detr_amd import datapath as dp
        from uni3detr_amd.schedule import StepSchedule
        from uni3detr_amd.step_log import StepLog
        from uni3detr_amd.trainer import TrainStep, plan_point_capacity
        from uni3detr_amd.training import EpochPlan, seed_epoch
        self.dev, self.samples = dev, samples
        self.pipe = dp.DevicePipeline(TRAIN_PIPELINE, load=True)
        self.plan = EpochPlan(len(SIZES), B, seed=0)
        assert self.plan.iters_per_epoch == IPE
        self.schedule = StepSchedule(2e-4, step=[1], gamma=0.1, iters_per_epoch=IPE)          # the lr drops at the second epoch
        self.model = _model(dev, sd)
        seed_epoch(0, 0, 0)
        with self.make_feeder(self.plan.order(0)) as f:
            first = list(f)
        self.P = plan_point_capacity([b["count"].tolist() for b in first])
        assert max(SIZES) <= self.P < BIG
        self.log = StepLog(capacity=16, device=dev)
        self.ts = TrainStep(self.model, *dp.unpack_batch(first[0]), graph=True, lr=2e-4, point_capacity=self.P, log=self.log, check_every=1000)
        self.ts.capture(batches=first)
        torch.cuda.synchronize()
        assert len(self.log) == 0                               # the capture's own steps are taken back out of the log
        self.snap = self.ts.snapshot_full()

    def make_feeder(self, order, samples=None):
        from uni3detr_amd.feeder import BatchFeeder
        return BatchFeeder(samples or self.samples, order, self.pipe, batch_size=B, device=self.dev, box_type_3d="Depth")

    def reset(self):
        self.ts.restore_full(self.snap)
        self.ts._buf.ingest_over.zero_()
        self.ts._steps_since_check = 0
        torch.cuda.synchronize()

    def fit(self, max_epochs=EPOCHS, **kw):
        from uni3detr_amd.training import fit
        kw.setdefault("printer", lambda s: None)
        kw.setdefault("make_feeder", self.make_feeder)
        return fit(self.ts, kw.pop("make_feeder"), self.plan, self.schedule, max_epochs, log_interval=2, **kw)

    def state(self):
        ts = self.ts
        return dict(param=ts.flat_param.clone(), m=ts.exp_avg.clone(), v=ts.exp_avg_sq.clone(), steps=float(ts.opt_state[0].item()),
                    buffers=[b.clone() for b in self.model.buffers()], rows=self.log.rows(0, len(self.log)))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from uni3detr_amd.datasets import samples_from_cfg
    root = str(tmp_path_factory.mktemp("sunrgbd"))
    ann, big = _write_dataset(root)
    cfg = dict(type="SUNRGBDDataset", data_root=root, ann_file=ann, pipeline=TRAIN_PIPELINE, filter_empty_gt=False, box_type_3d="Depth")
    samples, meta = samples_from_cfg(cfg)
    with_big, _ = samples_from_cfg(dict(cfg, ann_file=big))
    val, val_meta = samples_from_cfg(dict(cfg, pipeline=TEST_PIPELINE, test_mode=True))
    return dict(root=root, ann=ann, samples=samples, meta=meta, with_big=with_big, val=val, val_meta=val_meta)


@pytest.fixture(scope="module")
def runs(cuda, data):
    a = _Run(cuda, data["samples"])
    b = _Run(cuda, data["samples"], sd=copy.deepcopy({k: v.cpu() for k, v in a.model.state_dict().items()}))
    a.reset(); b.reset()
    return a, b


@pytest.fixture(scope="module")
def whole(runs):
    """2 uninterrupted epochs on the first run: what the other tests compare with"""
    a, _ = runs
    a.reset()
    out = a.fit()
    assert out["epoch"] == EPOCHS and out["iter"] == EPOCHS * IPE
    return dict(a.state(), records=out["records"])


def _same(x, y, what):
    d = (x.double() - y.double()).abs().max().item() if x.numel() else 0.0
    print(f"{what}: max |difference| {d:.3e}")
    assert torch.equal(x, y), (what, d)


def test_log_rows_equal_what_item_reads_per_step(runs, whole):
    """(i) every row of the log = what an identical second run reads with .item() after each step, bit for bit"""
    from uni3detr_amd import schedule as S
    from uni3detr_amd.step_log import STEP_LOG_FIXED
    from uni3detr_amd.training import seed_epoch
    a, b = runs
    b.reset()
    seen, it = [], 0
    for epoch in range(EPOCHS):
        seed_epoch(0, epoch, 0)
        with b.make_feeder(b.plan.order(epoch)) as f:
            for batch in f:
                S.apply(b.ts, b.schedule, it)
                with _no_host_sync():
                    b.ts.set_packed_batch(batch)
                    b.ts.step()                                 # the log is on: the step itself still reads nothing
                seen.append(dict(total=b.ts.loss.item(), terms=[v.item() for v in b.ts._losses.values()], norm=b.ts.opt_state[4].item(),
                                 coef=b.ts.opt_state[1].item(), lr=b.ts.opt_state[5].item(), beta1=b.ts.opt_state[6].item()))
                it += 1
    rows = whole["rows"]
    assert rows.shape == (EPOCHS * IPE, STEP_LOG_FIXED + 12) and a.log.names == list(b.ts._losses)
    assert rows[:, 0].tolist() == list(range(EPOCHS * IPE)) and rows[:, 1].tolist() == [1] * (EPOCHS * IPE) and not rows[:, 7].any()
    f = rows.view(np.float32)
    for k, s in enumerate(seen):
        got = dict(total=float(f[k, 2]), terms=f[k, STEP_LOG_FIXED:].astype(np.float64).tolist(), norm=float(f[k, 3]), coef=float(f[k, 4]),
                   lr=float(f[k, 5]), beta1=float(f[k, 6]))
        dev = max(abs(x - y) / max(abs(y), 1e-30) for x, y in zip([got["total"], got["norm"], got["coef"]] + got["terms"],
                                                                  [s["total"], s["norm"], s["coef"]] + s["terms"]))
        print("step", k, "log", got["total"], got["norm"], got["lr"], "item()", s["total"], s["norm"], s["lr"], "largest relative deviation", dev)
        assert got == s, (k, got, s)
        assert s["lr"] == float(np.float32(b.schedule.lr(k))) and np.isfinite(s["total"]) and s["total"] > 0
    assert f[0, 5] != f[IPE, 5]                                 # the schedule's step at the second epoch is in the log
    # the lines fit printed: windows of 2 and 1 steps per epoch, means of the rows above
    recs = [r for r in whole["records"] if r["mode"] == "train"]
    assert [(r["epoch"], r["iter"]) for r in recs] == [(1, 2), (1, 3), (2, 2), (2, 3)]
    assert recs[0]["loss"] == float(np.float32((np.float64(f[0, 2]) + np.float64(f[1, 2])) / 2)) and recs[1]["loss"] == float(f[2, 2])
    assert recs[0]["held"] == recs[0]["dropped"] == recs[0]["nonfinite"] == 0 and recs[0]["ms_per_step"] > 0


def test_resume_equals_uninterrupted(runs, whole, tmp_path):
    """(ii) 1 epoch + checkpoint + another step object + resume + 1 epoch = 2 uninterrupted epochs"""
    a, b = runs
    a.reset()
    out = a.fit(max_epochs=1, work_dir=str(tmp_path))
    assert out["epoch"] == 1 and sorted(os.listdir(tmp_path)) == ["epoch_1.pth", "latest.pth", "log.json"]
    b.reset()                                                   # the other model, step and log, at their initial state
    out = b.fit(resume=str(tmp_path / "latest.pth"), work_dir=str(tmp_path / "resumed"))
    assert out["epoch"] == EPOCHS and out["iter"] == EPOCHS * IPE
    assert [(r["epoch"], r["iter"]) for r in out["records"]] == [(2, 2), (2, 3)]
    got = b.state()
    _same(got["param"], whole["param"], "parameters")
    _same(got["m"], whole["m"], "exp_avg")
    _same(got["v"], whole["v"], "exp_avg_sq")
    assert got["steps"] == whole["steps"] == EPOCHS * IPE
    for x, y in zip(got["buffers"], whole["buffers"]):
        assert torch.equal(x, y)
    assert np.array_equal(got["rows"], whole["rows"])


def test_evaluate_hook_leaves_training_untouched(runs, whole, data):
    """(iii) a validation pass after epoch 1 changes neither the final parameters nor the BatchNorm buffers"""
    from uni3detr_amd.train import make_evaluate
    a, b = runs
    b.reset()
    ev = make_evaluate(data["val"], data["val_meta"], TEST_PIPELINE, B, b.dev, seed=0)
    seen = {}

    def hook(ts, epoch):
        if epoch != 1:
            return {}
        before = [x.clone() for x in b.model.buffers()]
        seen.update(ev(ts, epoch))
        assert b.model.training and all(torch.equal(x, y) for x, y in zip(before, b.model.buffers()))
        return seen
    out = b.fit(evaluate=hook, eval_interval=1)
    assert "mAP_0.25" in seen and "mAP_0.50" in seen and 0.0 <= seen["mAP_0.25"] <= 1.0
    val = [r for r in out["records"] if r["mode"] == "val"]
    assert len(val) == 2 and val[0]["epoch"] == 1 and val[0]["mAP_0.25"] == seen["mAP_0.25"]
    got = b.state()
    _same(got["param"], whole["param"], "parameters")
    for x, y in zip(got["buffers"], whole["buffers"]):
        assert torch.equal(x, y)
    assert np.array_equal(got["rows"], whole["rows"])


def test_batch_over_capacity_is_held_logged_and_reported(runs, data):
    """(iv) a scene above point_capacity: outcome 3 in the log, outside the window, raised by fit with its epoch and iteration"""
    a, b = runs
    b.reset()
    big = len(SIZES)                                            # the 6 000-point scene's index in `with_big`

    def make_feeder(order):
        return b.make_feeder([big if j == 4 else int(k) for j, k in enumerate(order)], samples=data["with_big"])       # in the third batch
    w0 = b.ts.flat_param.clone()
    with pytest.raises(RuntimeError, match=r"epoch 1 iteration 3: ingest overflow: 1 step\(s\) were held") as e:
        b.fit(make_feeder=make_feeder)
    assert "point_capacity" in str(e.value)
    rows = b.log.rows(0, len(b.log))
    assert rows[:, 1].tolist() == [1, 1, 3] and b.ts.applied_updates() == 2 and not torch.equal(w0, b.ts.flat_param)
    f = rows.view(np.float32)
    w = b.log.window(3)
    assert (w["steps"], w["held"], w["used"], w["nonfinite"]) == (3, 1, 2, 0)
    assert w["loss"] == float(np.float32((np.float64(f[0, 2]) + np.float64(f[1, 2])) / 2))
    last = b.log.window(1)
    assert (last["held"], last["used"], last["loss"]) == (1, 0, 0.0) and b.log.window(2)["used"] == 1


def test_command_line_trains_one_epoch(cuda, data, tmp_path):
    """(v) python -m uni3detr_amd.train CONFIG, in-process: 1 epoch on the synthetic set, --no-validate"""
    from uni3detr_amd import train
    cfg_path = tmp_path / "tiny_sunrgbd.py"
    train_set = dict(type="RepeatDataset", times=1, dataset=dict(type="SUNRGBDDataset", data_root=data["root"], ann_file=data["ann"],
                                                                 pipeline=TRAIN_PIPELINE, filter_empty_gt=False, box_type_3d="Depth"))
    cfg_path.write_text("\n".join([
        f"model = {tiny_cfg()!r}",
        f"train_pipeline = {TRAIN_PIPELINE!r}",
        f"test_pipeline = {TEST_PIPELINE!r}",
        f"data = dict(samples_per_gpu={B}, workers_per_gpu=0, train={train_set!r})",
        "optimizer = dict(type='AdamW', lr=2e-4, weight_decay=0.01)",
        "optimizer_config = dict(grad_clip=dict(max_norm=10, norm_type=2))",
        "lr_config = dict(policy='step', step=[1])",
        "runner = dict(type='EpochBasedRunner', max_epochs=3)",
        "evaluation = dict(interval=1)", ""]))
    work = tmp_path / "work"
    out = train.main([str(cfg_path), "--work-dir", str(work), "--max-epochs", "1", "--no-validate", "--log-interval", "2", "--seed", "0"])
    assert out["epoch"] == 1 and out["iter"] == IPE
    assert sorted(os.listdir(work)) == ["epoch_1.pth", "latest.pth", "log.json"]
    recs = [json.loads(l) for l in open(work / "log.json")]
    assert [(r["epoch"], r["iter"]) for r in recs] == [(1, 2), (1, 3)]
    assert all(np.isfinite(r["loss"]) and r["loss"] > 0 and r["lr"] == float(np.float32(2e-4)) and "d0.loss_cls" in r for r in recs)
    ck = torch.load(work / "latest.pth", weights_only=True)
    assert ck["meta"]["epoch"] == 1 and ck["meta"]["iter"] == IPE and ck["step_log"]["cursor"] == IPE and ck["optimizer"]["kind"] == "flat"
