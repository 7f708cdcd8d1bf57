"""LoadPointsFromFile on the device and the BatchFeeder at the SUN RGB-D shape (GPU box; not part of bench.py).

8 scenes x 50 000 x 6 raw rows per batch, the shipped SUN RGB-D train pipeline with PointSample(20000), the SUN RGB-D model:
  (a) the device load per batch - upload (wall clock around pack_batch(None, raw=...), synchronised) and kernels (device events around
      the LoadPointsFromFile transform: select + gather) - against the NumPy restatement (tests/load_ref.py: gather, percentile,
      concatenate, one scene at a time), same rows;
  (b) ms per captured training step three ways, each as (wall clock of --steps steps ending in one synchronise) / steps: resident
      batches (set_packed_batch of batches already in HBM), a synchronous feed (read files, pack, pipeline, then the step, on one
      stream) and the BatchFeeder over the same files and order;
  (c) the floor select alone, as u3d_points_load with shift_height minus the same call without it (the gather is in both), device
      events, at 8 x 50 000 rows and at 1 x 1 000 000 rows.

    python tools/load_bench.py [--scenes 8] [--rows 50000] [--batches 4] [--steps 40] [--warmup 5] [--iters 20] [--out FILE]

Prints one JSON line (and writes it to --out)."""
import argparse
import copy
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import load_ref as R  # noqa: E402
import projects.mmdet3d_plugin  # noqa: E402,F401
from uni3detr_amd import datapath as dp  # noqa: E402
from uni3detr_amd import native as nv  # noqa: E402
from uni3detr_amd.configs import pipelines as P  # noqa: E402
from uni3detr_amd.configs.sunrgbd import model as MODEL_CFG  # noqa: E402
from uni3detr_amd.feeder import BatchFeeder  # noqa: E402
from uni3detr_amd.registry import build_model  # noqa: E402
from uni3detr_amd.synth import room_scene  # noqa: E402
from uni3detr_amd.trainer import TrainStep  # noqa: E402

NUM_POINTS = 20000


def pipeline_cfg():
    cfg = copy.deepcopy(P.SHIPPED["sunrgbd"]["train_pipeline"])
    for c in cfg:
        if c["type"] == "LoadPointsFromFile":
            c.update(dp.SHIPPED_LOAD_ENTRIES["sunrgbd"])
        if c["type"] == "PointSample":
            c["num_points"] = NUM_POINTS
    return cfg


def events_ms(fn, iters):
    out = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def select_alone(scenes, rows, dev, iters):
    rng = np.random.default_rng(5)
    raw = rng.uniform(-3, 3, (scenes * rows, 6)).astype(np.float32)
    raw[:, 2] = rng.normal(0.3, 0.9, scenes * rows)
    raw_d = torch.from_numpy(raw).to(dev)
    off = torch.arange(0, (scenes + 1) * rows, rows, dtype=torch.int32, device=dev)
    tab = torch.from_numpy(dp.load_table([rows] * scenes)).to(dev)
    for _ in range(3):
        pts, fl = nv.points_load(raw_d, off, tab, [0, 1, 2], True)
        nv.points_load(raw_d, off, None, [0, 1, 2], False)
    assert R.same(fl.cpu().numpy(), np.array([R.floor_height(raw[b * rows:(b + 1) * rows, 2]) for b in range(scenes)], np.float32))
    with_h = events_ms(lambda: nv.points_load(raw_d, off, tab, [0, 1, 2], True), iters)
    without = events_ms(lambda: nv.points_load(raw_d, off, None, [0, 1, 2], False), iters)
    return dict(scenes=scenes, rows=rows, load_with_height_ms=round(with_h, 4), gather_only_ms=round(without, 4),
                select_ms=round(with_h - without, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "load_bench measures the device path: it needs the GPU"
    dev = torch.device("cuda:0")
    B = a.scenes
    rng = np.random.default_rng(0)
    np.random.seed(0)
    tmp = tempfile.mkdtemp(prefix="load_bench_")
    samples = []
    for k in range(a.batches * B):
        p, g, l = room_scene(k, a.rows)
        raw = np.concatenate([p[:, :3], rng.integers(0, 256, (a.rows, 3)).astype(np.float32)], 1)
        path = os.path.join(tmp, f"scan{k}.bin")
        raw.tofile(path)
        g = g.copy()
        g[:, 2] -= g[:, 5] / 2
        samples.append(dict(pts_filename=path, gt_bboxes_3d=g.astype(np.float32), gt_labels_3d=(l % 10).astype(np.int64)))
    cfg = pipeline_cfg()
    pipe = dp.DevicePipeline(cfg, load=True)
    entry = pipe.load_cfg

    def feed(idx, pp=pipe):
        recs = [dp.read_points(samples[k], entry) for k in idx]
        return pp(dp.pack_batch(None, [samples[k]["gt_bboxes_3d"] for k in idx], "Depth",
                                gt_labels_3d=[samples[k]["gt_labels_3d"] for k in idx], raw=recs, device=dev))

    # ---- (a) the load per batch ----
    recs0 = [dp.read_points(samples[k], entry) for k in range(B)]
    loader = dp.OBJECT_AUG.build(entry)
    for _ in range(3):
        loader(dp.pack_batch(None, raw=recs0, device=dev))
    torch.cuda.synchronize()
    up, kern = [], []
    for _ in range(a.iters):
        t0 = time.perf_counter()
        b = dp.pack_batch(None, raw=recs0, device=dev)
        torch.cuda.synchronize()
        up.append((time.perf_counter() - t0) * 1e3)
        kern.append(events_ms(lambda b=b: loader(dict(b)), 1))
    host = []
    for _ in range(max(3, a.iters // 4)):
        t0 = time.perf_counter()
        for r in recs0:
            R.load_points(r["raw"], entry["use_dim"], True)
        host.append((time.perf_counter() - t0) * 1e3)
    load = dict(upload_ms=round(statistics.median(up), 3), kernels_ms=round(statistics.median(kern), 4),
                host_restatement_ms=round(statistics.median(host), 3), raw_rows=B * a.rows)

    # ---- (b) the captured step, three feeds ----
    order = [k for _ in range((a.warmup + a.steps) // a.batches + 2) for k in range(a.batches * B)]
    resident = [feed(list(range(i * B, (i + 1) * B))) for i in range(a.batches)]
    torch.manual_seed(0)
    model = build_model(copy.deepcopy(MODEL_CFG)).to(dev).train()
    model.set_precision("bf16")
    ts = TrainStep(model, *dp.unpack_batch(resident[0]), graph=True, point_capacity=NUM_POINTS, check_every=0)
    ts.capture(batches=resident)

    def run_resident(n):
        for i in range(n):
            ts.set_packed_batch(resident[i % a.batches])
            ts.step()

    def run_sync(n):
        for i in range(n):
            ts.set_packed_batch(feed(order[i * B:(i + 1) * B]))
            ts.step()

    def run_feeder(n):
        with BatchFeeder(samples, order[:n * B], dp.DevicePipeline(cfg, load=True), batch_size=B, device=dev) as f:
            for batch in f:
                ts.set_packed_batch(batch)
                ts.step()

    def per_step(fn):
        fn(a.warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(a.steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    rounds = dict(resident=[], synchronous=[], feeder=[])
    for _ in range(3):                                  # alternating, three rounds each: the spread is in the output
        for name, fn in (("resident", run_resident), ("synchronous", run_sync), ("feeder", run_feeder)):
            rounds[name].append(per_step(fn))
    step = {k: round(statistics.median(v), 3) for k, v in rounds.items()}
    step["rounds"] = {k: [round(x, 3) for x in v] for k, v in rounds.items()}
    step["held_steps"], step["recaptures"] = ts.held_steps(), ts.recaptures

    out = dict(metric="device_load", scenes=B, rows=a.rows, num_points=NUM_POINTS, steps=a.steps, load_per_batch=load,
               captured_step_ms=step, select=[select_alone(B, a.rows, dev, a.iters), select_alone(1, 1_000_000, dev, a.iters)])
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
