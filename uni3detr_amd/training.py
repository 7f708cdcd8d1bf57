"""The epoch driver: what composes the captured step, the feeder, the schedules, the checkpoints, EMA and the evaluators into a training
run (ref: extra_tools/train.py and the mmcv EpochBasedRunner behind it, whose hooks this restates as one loop).

    plan = EpochPlan(len(samples), batch_size=B, repeat=5)
    fit(ts, lambda order: BatchFeeder(samples, order, pipe, batch_size=B), plan, build_schedule(cfg, plan.iters_per_epoch), max_epochs,
        work_dir="work_dirs/run", evaluate=hook, eval_interval=2)

The loop never waits for the host inside an epoch: the losses of every step go into the step's device-side log (step_log.StepLog, written
inside the captured graph) and are read once per `log_interval` steps, when a line is printed.

Randomness.  At the start of every epoch np.random and torch are seeded from (seed, epoch, rank); the order of the epoch is a function of
(plan.seed, epoch).  A feeder started from a given np.random state yields bit-identical batches (feeder.py), so an epoch is a function of
its number and of the state it starts from - which is why checkpoints are taken at epoch boundaries only: inside an epoch the feeder has
drawn for batches the step has not consumed yet, and the random state of that moment is not the consumed batches' state.
"""
import json
import os
import shutil
import time

import numpy as np
import torch

from . import schedule as _schedule
from .checkpoint import _load_file, load_checkpoint, save_checkpoint


class EpochPlan:
    """Which sample indices a rank sees in which epoch: what mmdet's RepeatDataset, mmdet3d's CBGSDataset and the distributed sampler
    decide between them (feeder.py leaves all three with the caller).  Pure numpy, no device.

    repeat: the index list concatenated `repeat` times (RepeatDataset).  class_ids: one list of category ids per sample (the reference's
    get_cat_ids: the names of the sample's boxes - the valid ones with use_valid_flag - mapped to class ids, each once) - the
    class-balanced resampling of CBGSDataset: per-class index lists, class c drawn int(len_c * (1 / n_classes) / share_c) times with
    replacement, share_c = len_c / sum of the lengths.  The draw comes from an np.random.RandomState(seed) of the plan's own and happens
    once, at construction.  Parity with upstream: unpinned - mmdet3d's draw order (np.random.choice per class, in class order, from the
    global generator) is restated from memory of its definition, not checked against its source, and its generator state is whatever
    the process had.
    order(epoch): a permutation seeded by seed + epoch, padded by wrap-around to a multiple of world * batch_size, of which rank r takes
    every world-th index starting at r (DistributedSampler's rule)."""

    def __init__(self, n_samples, batch_size, world=1, rank=0, seed=0, repeat=1, class_ids=None, shuffle=True):
        self.n_samples, self.batch_size, self.world, self.rank = int(n_samples), int(batch_size), int(world), int(rank)
        self.seed, self.repeat, self.shuffle = int(seed), int(repeat), bool(shuffle)
        if self.n_samples < 1 or self.batch_size < 1 or self.world < 1 or self.repeat < 1 or not 0 <= self.rank < self.world:
            raise ValueError("EpochPlan: n_samples, batch_size, world, repeat >= 1 and 0 <= rank < world")
        base = np.arange(self.n_samples, dtype=np.int64)
        self.cbgs = class_ids is not None
        if self.cbgs:
            if len(class_ids) != self.n_samples:
                raise ValueError(f"EpochPlan: {len(class_ids)} class-id lists for {self.n_samples} samples")
            base = self._class_balanced(class_ids)
        self.base = np.tile(base, self.repeat)
        if self.base.size == 0:
            raise ValueError("EpochPlan: the class-balanced resampling left no sample (no sample has a box of a known class)")
        group = self.world * self.batch_size
        self.iters_per_epoch = (self.base.size + group - 1) // group

    def _class_balanced(self, class_ids):
        per_class = {}
        for i, ids in enumerate(class_ids):
            for c in sorted({int(c) for c in ids}):
                per_class.setdefault(c, []).append(i)
        classes = sorted(per_class)
        n_classes = len(classes)           # (upstream divides by the share of every class of CLASSES: it needs all of them present)
        dup = sum(len(per_class[c]) for c in classes)
        rng = np.random.RandomState(self.seed)
        out = []
        for c in classes:
            idx = per_class[c]
            share = len(idx) / dup
            out += rng.choice(idx, int(len(idx) * (1.0 / n_classes) / share)).tolist()
        return np.asarray(out, dtype=np.int64)

    def __len__(self):
        return int(self.base.size)

    def global_order(self, epoch, pad=True):
        """The job's index list of `epoch` before it is dealt to the ranks; pad: wrapped around to a multiple of world * batch_size."""
        idx = self.base
        if self.shuffle:
            idx = idx[np.random.RandomState(self.seed + int(epoch)).permutation(idx.size)]
        if pad:
            total = self.iters_per_epoch * self.world * self.batch_size
            idx = np.resize(idx, total)             # (np.resize repeats from the start: wrap-around)
        return idx

    def order(self, epoch, rank=None):
        """The indices of rank `rank` (default: the plan's own) in `epoch`: iters_per_epoch * batch_size of them."""
        return self.global_order(epoch)[(self.rank if rank is None else int(rank))::self.world]

    def params(self):
        """What a checkpoint's meta records of the plan (a resume refuses another plan)."""
        return dict(n_samples=self.n_samples, batch_size=self.batch_size, world=self.world, seed=self.seed, repeat=self.repeat,
                    shuffle=self.shuffle, cbgs=self.cbgs, length=len(self), iters_per_epoch=self.iters_per_epoch)


def seed_epoch(seed, epoch, rank):
    """The per-epoch seeding rule: np.random (the feeder's and the pipelines' draws) and torch (dropout) from (seed, epoch, rank)."""
    np.random.seed([int(seed) & 0xFFFFFFFF, int(epoch), int(rank)])
    torch.manual_seed((int(seed) * 1000003 + int(epoch)) * 1009 + int(rank))


def _line(rec):
    if rec["mode"] == "val":
        return f"Epoch(val) [{rec['epoch']}]  " + ", ".join(f"{k}: {v:.4f}" if isinstance(v, float) else f"{k}: {v}"
                                                          for k, v in rec.items() if k not in ("mode", "epoch", "iter"))
    head = f"Epoch [{rec['epoch']}][{rec['iter']}/{rec['iters_per_epoch']}]  "
    skip = ("mode", "epoch", "iter", "iters_per_epoch", "global_iter")
    return head + ", ".join(f"{k}: {v:.3e}" if k == "lr" else f"{k}: {v:.4f}" if isinstance(v, float) else f"{k}: {v}"
                            for k, v in rec.items() if k not in skip)


def _bind(ts, batch):
    if getattr(ts, "point_capacity", 0) is None:      # the fixed layout (dynamic voxelization behind PointSample): lists through set_batch
        from . import datapath as dp
        ts.set_batch(*dp.unpack_batch(batch))
    else:
        ts.set_packed_batch(batch)


def fit(ts, make_feeder, plan, schedule, max_epochs, *, log=None, log_interval=50, work_dir=None, checkpoint_interval=1, evaluate=None,
        eval_interval=0, resume=None, seed=0, max_iters=None, printer=print):
    """Train `ts` (a TrainStep, captured or eager) for epochs [start, max_epochs) of `plan`.

    make_feeder(order) -> an iterable context manager of packed batches (feeder.BatchFeeder) over the epoch's indices.  Per batch:
    schedule.apply(ts, schedule, it) with `it` counting steps from the run's first epoch, ts.set_packed_batch(batch), ts.step().
    log (default ts.log): every `log_interval` steps of an epoch - and at its last step - log.window() over the steps since the last
    line is read (the loop's only device-to-host read), printed through `printer` and appended as a JSON line to work_dir/log.json;
    a window in which every total loss is non-finite raises FloatingPointError.  Held steps are counted in the line; when the step
    reports cut batches (ingest_overflows()) the error it would raise at its periodic check is raised here, with the epoch and iteration
    of the first held step added, as is any RuntimeError out of step() itself.
    Every `checkpoint_interval` epochs epoch_{k}.pth and a copy latest.pth are written to work_dir: the model,
    ts.optimizer_state_dict() (moments, step state, open window, EMA weights), the log's state and meta = epoch, iter, seed, plan.
    evaluate(ts, epoch) -> metrics dict, every `eval_interval` epochs (k counted from 1), inside ts.ema_scope() when EMA is on.
    resume: a checkpoint of this function; everything above is restored and the run continues at the next epoch.
    max_iters: stop after that many steps of this call (mid-epoch: no checkpoint is written for the unfinished epoch).
    -> dict(epoch = epochs completed, iter = steps since the run's start, records = the logged dicts)."""
    log = getattr(ts, "log", None) if log is None else log
    log_interval = max(1, int(log_interval))
    rank, ipe = plan.rank, plan.iters_per_epoch
    start_epoch, it = 0, 0
    if resume is not None:
        ck = _load_file(resume, "cpu")
        meta = ck["meta"]
        if meta.get("plan") != plan.params():
            raise ValueError(f"resume: {resume} was written for the plan {meta.get('plan')}, this run's is {plan.params()}")
        load_checkpoint(ts.model, ck, strict=True)
        ts.load_optimizer_state_dict(ck["optimizer"])
        if log is not None and ck.get("step_log") is not None:
            log.load_state_dict(ck["step_log"])
        start_epoch, it, seed = int(meta["epoch"]), int(meta["iter"]), int(meta["seed"])
    log_path = None
    if work_dir is not None and rank == 0:
        os.makedirs(work_dir, exist_ok=True)
        log_path = os.path.join(work_dir, "log.json")
    records, done = [], 0

    def emit(rec):
        records.append(rec)
        if rank == 0:
            printer(_line(rec))
            if log_path is not None:
                with open(log_path, "a") as f:
                    f.write(json.dumps(rec) + "\n")

    def report(epoch, i, n, t0):
        """the line after step i (0-based) of `epoch`, over the last n steps"""
        rec = dict(mode="train", epoch=epoch + 1, iter=i + 1, iters_per_epoch=ipe, global_iter=it)
        w = None if log is None else log.window(n)         # (synchronises: the wall clock below covers finished steps)
        rec.update({k: v for k, v in (w or {}).items() if k not in ("steps", "used")})
        rec["ms_per_step"] = (time.perf_counter() - t0) * 1e3 / n
        emit(rec)
        if w is not None:
            if w["used"] == 0 and w["nonfinite"] > 0:
                raise FloatingPointError(f"epoch {epoch + 1} iteration {i + 1}: the total loss of all {w['nonfinite']} step(s) since the "
                                         "last line is NaN / Inf")
            if w["held"] > 0 and getattr(ts, "ingest_overflows", lambda: 0)() > 0:
                rows = log.rows(len(log) - n, n)
                first = it - n + int(np.flatnonzero(rows[:, 1] == 3)[0])
                try:
                    ts._raise_on_ingest_overflow()
                except RuntimeError as e:
                    raise RuntimeError(f"epoch {first // ipe + 1} iteration {first % ipe + 1}: {e}") from e

    epoch = start_epoch
    for epoch in range(start_epoch, int(max_epochs)):
        seed_epoch(seed, epoch, rank)
        since, t0, stopped = 0, time.perf_counter(), False
        with make_feeder(plan.order(epoch)) as feeder:
            for i, batch in enumerate(feeder):
                _schedule.apply(ts, schedule, it)
                _bind(ts, batch)
                try:
                    ts.step()
                except RuntimeError as e:
                    raise RuntimeError(f"epoch {epoch + 1} iteration {i + 1}: {e}") from e
                it, done, since = it + 1, done + 1, since + 1
                last = max_iters is not None and done >= int(max_iters)
                if since == log_interval or i + 1 == ipe or last:
                    report(epoch, i, since, t0)
                    since, t0 = 0, time.perf_counter()
                if last:
                    stopped = i + 1 < ipe
                    break
        if stopped:
            return dict(epoch=epoch, iter=it, records=records)
        k = epoch + 1
        if work_dir is not None and rank == 0 and checkpoint_interval and k % int(checkpoint_interval) == 0:
            path = os.path.join(work_dir, f"epoch_{k}.pth")
            save_checkpoint(ts.model, path, meta=dict(epoch=k, iter=it, seed=int(seed), plan=plan.params()),
                            optimizer_state=ts.optimizer_state_dict(), extra=dict(step_log=None if log is None else log.state_dict()))
            shutil.copyfile(path, os.path.join(work_dir, "latest.pth"))
        if evaluate is not None and eval_interval and k % int(eval_interval) == 0:
            if getattr(ts, "ema", None) is not None:
                with ts.ema_scope():
                    metrics = evaluate(ts, k)
            else:
                metrics = evaluate(ts, k)
            emit(dict(mode="val", epoch=k, iter=it, **{m: (float(v) if isinstance(v, (int, float, np.floating)) else v)
                                                       for m, v in (metrics or {}).items()}))
        if max_iters is not None and done >= int(max_iters):
            return dict(epoch=k, iter=it, records=records)
    return dict(epoch=max(start_epoch, int(max_epochs)), iter=it, records=records)
