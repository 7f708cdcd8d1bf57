"""training.EpochPlan (pure numpy) and training.fit with CPU stand-ins for the step, the feeder and the log: the call order, the
iteration count the schedule sees, checkpoints, resume, max_iters and the non-finite stop - no device involved."""
import json
import os

import numpy as np
import pytest
import torch

from uni3detr_amd import training as T
from uni3detr_amd.feeder import BatchFeeder


# ---- EpochPlan ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, B, world, repeat", [(10, 3, 1, 1), (10, 3, 2, 2), (7, 2, 3, 5), (4, 8, 2, 1)])
def test_plan_covers_every_index_and_ranks_partition(n, B, world, repeat):
    plan = T.EpochPlan(n, B, world=world, seed=3, repeat=repeat)
    assert len(plan) == n * repeat and plan.iters_per_epoch == -(-n * repeat // (world * B))
    raw = plan.global_order(0, pad=False)
    assert np.bincount(raw, minlength=n).tolist() == [repeat] * n                  # every index `repeat` times before padding
    padded = plan.global_order(0)
    assert padded.size == plan.iters_per_epoch * world * B and np.array_equal(padded[:raw.size], raw)
    assert np.array_equal(padded[raw.size:], np.resize(raw, padded.size)[raw.size:])      # wrap-around
    parts = [T.EpochPlan(n, B, world=world, rank=r, seed=3, repeat=repeat).order(0) for r in range(world)]
    assert all(p.size == plan.iters_per_epoch * B for p in parts)
    inter = np.empty(padded.size, np.int64)
    for r, p in enumerate(parts):
        inter[r::world] = p
    assert np.array_equal(inter, padded)                                           # the ranks deal the padded order out, nothing lost
    assert np.array_equal(plan.order(0, rank=world - 1), parts[-1])


def test_plan_epochs_differ_and_repeat():
    plan = T.EpochPlan(50, 4, seed=1)
    assert not np.array_equal(plan.order(0), plan.order(1))
    assert np.array_equal(plan.order(1), T.EpochPlan(50, 4, seed=1).order(1))
    assert np.array_equal(plan.order(1), T.EpochPlan(50, 4, seed=0).order(2))      # the permutation's seed is seed + epoch
    fixed = T.EpochPlan(6, 2, shuffle=False, repeat=2)
    assert fixed.order(0).tolist() == fixed.order(3).tolist() == [0, 1, 2, 3, 4, 5] * 2
    with pytest.raises(ValueError):
        T.EpochPlan(5, 2, world=2, rank=2)
    assert plan.params() == dict(n_samples=50, batch_size=4, world=1, seed=1, repeat=1, shuffle=True, cbgs=False, length=50,
                                 iters_per_epoch=13)


def test_plan_class_balanced():
    # 3 classes: class 0 in 12 samples, class 1 in 6, class 2 in 2 (sample 19 carries classes 1 and 2; sample 18 none)
    ids = [[0]] * 12 + [[1]] * 5 + [[2]] + [[]] + [[2, 1]]
    plan = T.EpochPlan(len(ids), 2, seed=5, class_ids=ids)
    per_class = {0: set(range(12)), 1: set(range(12, 17)) | {19}, 2: {17, 19}}
    dup = 12 + 6 + 2
    draws = int(dup / 3)                                       # int(len_c * (1 / 3) / (len_c / dup)) for every class
    assert len(plan) == 3 * draws
    base = plan.base
    for k, c in enumerate((0, 1, 2)):                          # drawn class by class, each `draws` times from its own list
        seg = base[k * draws:(k + 1) * draws]
        assert set(seg.tolist()) <= per_class[c]
        assert abs(seg.size / base.size - 1 / 3) <= 1 / base.size
    assert 18 not in base
    assert np.array_equal(base, T.EpochPlan(len(ids), 2, seed=5, class_ids=ids).base)
    assert not np.array_equal(base, T.EpochPlan(len(ids), 2, seed=6, class_ids=ids).base)
    assert plan.params()["cbgs"] and np.bincount(plan.global_order(0, pad=False), minlength=20).sum() == len(plan)
    with pytest.raises(ValueError):
        T.EpochPlan(3, 2, class_ids=ids)


# ---- fit with stand-ins -------------------------------------------------------------------------------------------------------------
class _Log:
    """what fit uses of step_log.StepLog, on the host"""

    def __init__(self):
        self.totals, self.outcomes = [], []

    def push(self, total, outcome=1):
        self.totals.append(float(total)); self.outcomes.append(int(outcome))

    def __len__(self):
        return len(self.totals)

    def window(self, last=50):
        t, o = np.asarray(self.totals[-last:]), np.asarray(self.outcomes[-last:])
        live = o != 3
        ok = live & np.isfinite(t)
        return dict(loss=float(t[ok].mean()) if ok.any() else 0.0, lr=1e-3, steps=int(t.size), held=int((~live).sum()), dropped=0,
                    nonfinite=int((live & ~np.isfinite(t)).sum()), used=int(ok.sum()))

    def rows(self, first, count):
        out = np.zeros((count, 9), np.int32)
        out[:, 1] = self.outcomes[first:first + count]
        return out

    def state_dict(self):
        return dict(totals=torch.tensor(self.totals, dtype=torch.float64), outcomes=list(self.outcomes))

    def load_state_dict(self, sd):
        self.totals, self.outcomes = sd["totals"].tolist(), list(sd["outcomes"])


class _Step:
    """what fit uses of trainer.TrainStep; every call is written into `calls`"""

    def __init__(self, calls, losses=None):
        self.model = torch.nn.Linear(2, 1)
        torch.nn.init.zeros_(self.model.weight); torch.nn.init.zeros_(self.model.bias)
        self.log, self.calls, self.losses = _Log(), calls, losses
        self.accum_steps, self.ema, self.steps, self.lr = 1, None, 0, None

    def set_hyper(self, lr=None, **kw):
        self.lr = lr
        self.calls.append(("hyper", lr))

    def set_packed_batch(self, batch):
        self.calls.append(("bind", batch["idx"]))

    def step(self):
        with torch.no_grad():
            self.model.weight += 1.0
        self.log.push(self.losses[self.steps] if self.losses is not None else 1.0 + self.steps)
        self.steps += 1
        self.calls.append(("step", self.steps))

    def optimizer_state_dict(self):
        return dict(kind="stand-in", steps=self.steps)

    def load_optimizer_state_dict(self, sd):
        self.steps = int(sd["steps"])


class _Schedule:
    def hyper(self, it):
        return dict(lr=float(it))                              # the iteration itself: set_hyper then shows what apply() saw


def _feeder_factory(calls, n, B):
    samples = [dict(pts_filename=str(k)) for k in range(n)]

    class Pipe:
        load_cfg = dict(type="LoadPointsFromFile")

        def __call__(self, batch):
            return batch

    def pack(points, gts, box_type, gt_labels_3d=None, raw=None, device=None):
        return dict(idx=[r["k"] for r in raw], draw=float(np.random.rand()))

    def make(order):
        calls.append(("feeder", list(map(int, order))))
        f = BatchFeeder(samples, order, Pipe(), batch_size=B, device="cpu", pack=pack)
        return f
    return make


@pytest.fixture
def host_reads(monkeypatch):
    from uni3detr_amd import datapath as dp
    monkeypatch.setattr(dp, "read_points", lambda sample, cfg: dict(k=int(sample["pts_filename"])))


def _run(tmp_path, calls, max_epochs, n=6, B=2, **kw):
    ts = kw.pop("ts", None) or _Step(calls)
    plan = T.EpochPlan(n, B, seed=2)
    lines = []
    out = T.fit(ts, _feeder_factory(calls, n, B), plan, _Schedule(), max_epochs, work_dir=str(tmp_path), printer=lines.append, **kw)
    return ts, plan, out, lines


def test_fit_call_order_iterations_and_checkpoints(tmp_path, host_reads):
    calls = []
    ts, plan, out, lines = _run(tmp_path, calls, 2, log_interval=2, checkpoint_interval=1)
    assert plan.iters_per_epoch == 3 and out["epoch"] == 2 and out["iter"] == 6
    feeders = [c for c in calls if c[0] == "feeder"]
    assert [f[1] for f in feeders] == [plan.order(0).tolist(), plan.order(1).tolist()]
    per_step = [c for c in calls if c[0] != "feeder"]
    assert [c[0] for c in per_step] == ["hyper", "bind", "step"] * 6                       # apply -> bind -> step, every iteration
    assert [c[1] for c in per_step if c[0] == "hyper"] == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]   # iterations count across epochs
    bound = [i for c in per_step if c[0] == "bind" for i in c[1]]
    assert bound == plan.order(0).tolist() + plan.order(1).tolist()
    assert sorted(os.listdir(tmp_path)) == ["epoch_1.pth", "epoch_2.pth", "latest.pth", "log.json"]
    ck = torch.load(tmp_path / "latest.pth", weights_only=True)
    assert ck["meta"] == dict(epoch=2, iter=6, seed=0, plan=plan.params()) and ck["optimizer"]["steps"] == 6
    assert ck["step_log"]["outcomes"] == [1] * 6 and torch.equal(ck["state_dict"]["weight"], ts.model.weight.detach())
    recs = [json.loads(l) for l in open(tmp_path / "log.json")]
    assert [(r["epoch"], r["iter"]) for r in recs] == [(1, 2), (1, 3), (2, 2), (2, 3)] and len(lines) == 4
    assert recs[0]["loss"] == 1.5 and recs[1]["loss"] == 3.0 and recs[3]["global_iter"] == 6 and recs[0]["ms_per_step"] >= 0
    assert lines[0].startswith("Epoch [1][2/3]") and "loss: 1.5000" in lines[0]


def test_fit_checkpoint_interval_and_eval_hook(tmp_path, host_reads):
    calls, seen = [], []

    def evaluate(ts, epoch):
        seen.append((epoch, ts.steps))
        return {"mAP_0.25": 0.5}
    ts, plan, out, lines = _run(tmp_path, calls, 3, checkpoint_interval=2, evaluate=evaluate, eval_interval=2)
    assert sorted(os.listdir(tmp_path)) == ["epoch_2.pth", "latest.pth", "log.json"] and seen == [(2, 6)]
    recs = [json.loads(l) for l in open(tmp_path / "log.json")]
    assert [r["mode"] for r in recs] == ["train", "train", "val", "train"] and recs[2]["mAP_0.25"] == 0.5 and recs[2]["epoch"] == 2


def test_fit_resume_continues_epoch_iteration_and_random_state(tmp_path, host_reads):
    whole_calls, a_calls, b_calls = [], [], []
    _run(tmp_path / "whole", whole_calls, 2)
    _run(tmp_path / "a", a_calls, 1)
    ts = _Step(b_calls)
    _, plan, out, _ = _run(tmp_path / "b", b_calls, 2, ts=ts, resume=str(tmp_path / "a" / "latest.pth"))
    assert out["epoch"] == 2 and out["iter"] == 6 and ts.steps == 6
    assert [c for c in b_calls if c[0] == "feeder"] == [("feeder", plan.order(1).tolist())]
    assert [c[1] for c in b_calls if c[0] == "hyper"] == [3.0, 4.0, 5.0]
    assert a_calls + b_calls == whole_calls
    a, b = (torch.load(tmp_path / d / "epoch_2.pth", weights_only=True) for d in ("whole", "b"))
    assert torch.equal(a["state_dict"]["weight"], b["state_dict"]["weight"]) and a["meta"] == b["meta"]
    assert torch.equal(a["step_log"]["totals"], b["step_log"]["totals"])
    with pytest.raises(ValueError, match="plan"):
        T.fit(_Step([]), _feeder_factory([], 8, 2), T.EpochPlan(8, 2, seed=2), _Schedule(), 2, resume=str(tmp_path / "a" / "latest.pth"),
              printer=lambda s: None)


def test_fit_epoch_seeding_makes_batches_a_function_of_the_epoch(tmp_path, host_reads):
    draws = []

    class Rec(_Step):
        def set_packed_batch(self, batch):
            draws.append(batch["draw"])
    _run(tmp_path / "x", [], 2, ts=Rec([]))
    first = list(draws)
    del draws[:]
    np.random.seed(99)                                          # whatever the process did before: the epoch seeds itself
    _run(tmp_path / "y", [], 2, ts=Rec([]))
    assert draws == first and len(set(first)) == 6
    del draws[:]
    _run(tmp_path / "z", [], 2, ts=Rec([]), seed=1)
    assert draws != first


def test_fit_max_iters_stops_mid_epoch_without_a_checkpoint(tmp_path, host_reads):
    calls = []
    ts, plan, out, lines = _run(tmp_path, calls, 2, max_iters=4)
    assert out["epoch"] == 1 and out["iter"] == 4 and ts.steps == 4
    assert sorted(os.listdir(tmp_path)) == ["epoch_1.pth", "latest.pth", "log.json"]
    recs = [json.loads(l) for l in open(tmp_path / "log.json")]
    assert [(r["epoch"], r["iter"]) for r in recs] == [(1, 3), (2, 1)]


def test_fit_raises_on_a_window_of_non_finite_totals(tmp_path, host_reads):
    ts = _Step([], losses=[1.0, float("nan"), 2.0, float("nan"), float("inf"), 3.0])
    with pytest.raises(FloatingPointError, match="epoch 2 iteration 2"):
        _run(tmp_path, [], 2, ts=ts, log_interval=2)            # windows: (1, nan) fine, (2) fine, (nan, inf) raises
    assert ts.steps == 5


def test_fit_adds_epoch_and_iteration_to_a_step_error(tmp_path, host_reads):
    class Bad(_Step):
        def step(self):
            if self.steps == 4:
                raise RuntimeError("ingest overflow: 1 step(s) were held")
            super().step()
    with pytest.raises(RuntimeError, match=r"epoch 2 iteration 2: ingest overflow"):
        _run(tmp_path, [], 2, ts=Bad([]))
