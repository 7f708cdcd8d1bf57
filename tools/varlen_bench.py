"""The captured training step on batches whose scenes differ in size (GPU box; not part of bench.py).

A nuScenes-shaped stream of batches - `synth.room_scene` scenes of drawn sizes in the nuScenes range, five point columns, 9-column
boxes, packed and range-filtered as a DevicePipeline leaves them - goes through
  (a) the captured capacity-mode step: TrainStep(point_capacity=P), set_packed_batch(batch) + step();
  (b) what the step could do with such batches before: datapath.unpack_batch (host reads) + an eager TrainStep(graph=False) whose
      buffers are re-bound from the lists (cheaper than the new TrainStep per batch its public interface asks for);
  (c) the captured fixed-size step on scenes of exactly P points, set_batch + step() - the cost of always padding to the capacity.
The three run alternately on the same batch index inside one loop, each between device synchronisations; the figures are medians.
The ingest alone is timed with device events.

    python tools/varlen_bench.py [--batch 2] [--batches 6] [--min-points 170000] [--max-points 250000] [--steps 20] [--warmup 3]

Prints the drawn sizes and one JSON line."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import projects.mmdet3d_plugin  # noqa: E402,F401
from uni3detr_amd import datapath as dp  # noqa: E402
from uni3detr_amd.configs import variants  # noqa: E402
from uni3detr_amd.plugin.structures import Boxes3D  # noqa: E402
from uni3detr_amd.registry import build_model  # noqa: E402
from uni3detr_amd.synth import room_scene  # noqa: E402
from uni3detr_amd.trainer import TrainStep, plan_point_capacity  # noqa: E402


def scenes(sizes, seed, dev):
    cfg = variants.nuscenes
    rng_range = tuple(cfg["pts_voxel_layer"]["point_cloud_range"])
    rng = np.random.default_rng(seed)
    pts, boxes, labels = [], [], []
    for i, n in enumerate(sizes):
        p, g, l = room_scene(seed * 64 + i, int(n), pc_range=rng_range)
        p = np.concatenate([p, rng.integers(0, 10, (p.shape[0], 1)).astype(np.float32) * np.float32(0.05)], 1)
        g = g.copy()
        g[:, 2] -= g[:, 5] / 2
        g = np.concatenate([g, rng.normal(0, 2, (g.shape[0], 2)).astype(np.float32)], 1)
        pts.append(torch.from_numpy(p).to(dev)); boxes.append(torch.from_numpy(g).to(dev))
        labels.append(torch.from_numpy((l % cfg["pts_bbox_head"]["num_classes"]).astype(np.int32)).to(dev))
    return pts, boxes, labels


def packed(sizes, seed, dev):
    pts, boxes, labels = scenes(sizes, seed, dev)
    batch = dp.pack_batch(pts, boxes, "LiDAR", gt_labels_3d=labels)
    return dp.PointsRangeFilter(list(variants.nuscenes["pts_voxel_layer"]["point_cloud_range"]))(batch)


def model(dev, sd=None):
    torch.manual_seed(0)
    m = build_model(copy.deepcopy(variants.nuscenes))
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(dev).train().set_precision("bf16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--min-points", type=int, default=170000)
    ap.add_argument("--max-points", type=int, default=250000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "varlen_bench needs the GPU"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    sizes = [[int(v) for v in rng.integers(a.min_points, a.max_points + 1, a.batch)] for _ in range(a.batches)]
    print("[varlen_bench] drawn scene sizes:", sizes, flush=True)
    stream = [packed(s, 100 + i, dev) for i, s in enumerate(sizes)]
    live = [b["count"].tolist() for b in stream]
    P = plan_point_capacity(live)
    print(f"[varlen_bench] live points per scene: {live}; point capacity P = {P}", flush=True)
    fixed = []
    for i in range(a.batches):
        p, g, l = scenes([P] * a.batch, 200 + i, dev)
        fixed.append((p, [Boxes3D(b) for b in g], [t.long() for t in l]))

    ma = model(dev)
    sd = copy.deepcopy(ma.state_dict())
    ts_a = TrainStep(ma, *dp.unpack_batch(stream[0]), graph=True, point_capacity=P, check_every=0)
    ts_a.capture(batches=stream)
    mb = model(dev, sd)
    ts_b = TrainStep(mb, *dp.unpack_batch(stream[0]), graph=False, check_every=0)
    mc = model(dev, sd)
    ts_c = TrainStep(mc, *fixed[0], graph=True, check_every=0)
    ts_c.capture(batches=fixed)

    def step_a(b):
        ts_a.set_packed_batch(b)
        return ts_a.step()

    def step_b(b):
        pts, gts, labels = dp.unpack_batch(b)
        ts_b.pts = mb.pack_points(pts)
        ts_b.gts = ts_b._pack_gts_static(gts, labels)
        return ts_b.step()

    def step_c(i):
        ts_c.set_batch(*fixed[i])
        return ts_c.step()

    def timed(fn, arg):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = fn(arg)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, float(loss)

    ms = dict(a=[], b=[], c=[])
    for it in range(a.warmup + a.steps):
        i = it % a.batches
        for key, fn, arg in (("a", step_a, stream[i]), ("b", step_b, stream[i]), ("c", step_c, i)):
            t, loss = timed(fn, arg)
            assert np.isfinite(loss), (key, it, loss)
            if it >= a.warmup:
                ms[key].append(t)
    ev = []
    for it in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ts_a.set_packed_batch(stream[it % a.batches])
        e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = dict(batch=a.batch, batches=a.batches, steps=a.steps, point_capacity=P, live_points=live,
               captured_capacity_ms=round(med["a"], 3), eager_unpack_ms=round(med["b"], 3), captured_fixed_P_ms=round(med["c"], 3),
               ingest_ms=round(statistics.median(ev), 4), ingest_rows=int(sum(live[0])),
               min_ms={k: round(min(v), 3) for k, v in ms.items()}, max_ms={k: round(max(v), 3) for k, v in ms.items()},
               held_steps=ts_a.held_steps(), ingest_overflows=ts_a.ingest_overflows(), recaptures=ts_a.recaptures,
               capacity_faster_than_eager=bool(med["a"] < med["b"]))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
