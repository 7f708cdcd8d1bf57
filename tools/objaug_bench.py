"""Device time of GT-paste (ObjectSample) + ObjectNoise on a KITTI-shaped batch against the NumPy host restatement of the same
steps (tests/objaug_ref.py, the per-sample work upstream runs in DataLoader workers), on the same draws.

    python tools/objaug_bench.py [--scenes 4] [--points 120000] [--db 2000] [--iters 20]

Prints one JSON line: device ms per batch (events around ObjectSample + ObjectNoise, draws and the one stats read included),
host ms per batch, and the counts behind them."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import objaug_ref as R  # noqa: E402
from uni3detr_amd import datapath as dp  # noqa: E402
from uni3detr_amd.gtdb import GTDatabase  # noqa: E402

CLASSES = ["Car", "Pedestrian", "Cyclist"]
SIZES = np.array([(3.9, 1.6, 1.5), (0.8, 0.6, 1.7), (1.8, 0.6, 1.7)], np.float32)
DB_SAMPLER = dict(rate=1.0, classes=CLASSES, sample_groups=dict(Car=20, Pedestrian=6, Cyclist=6))
NOISE = dict(type="ObjectNoise", num_try=100, translation_std=[1.0, 1.0, 0.5], global_rot_range=[0.0, 0.0], rot_range=[-0.78539816, 0.78539816])


def boxes(rng, n):
    lab = rng.choice(3, n, p=[0.7, 0.2, 0.1])
    b = np.zeros((n, 7), np.float32)
    b[:, 0], b[:, 1], b[:, 2] = rng.uniform(2, 68, n), rng.uniform(-36, 36, n), rng.uniform(-2, -1, n)
    b[:, 3:6] = SIZES[lab] * rng.uniform(0.9, 1.1, (n, 1))
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    return b, lab


def scene(rng, n, g):
    b, lab = boxes(rng, g)
    p = np.stack([rng.uniform(0, 70, n), rng.uniform(-40, 40, n), rng.uniform(-3, 1, n), rng.uniform(0, 1, n)], 1).astype(np.float32)
    return p, b, lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--db", type=int, default=2000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "objaug_bench measures the device path: it needs the GPU"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    np.random.seed(0)
    src = [scene(rng, 60000, a.db // 20) for _ in range(20)]
    db = GTDatabase.from_scenes([torch.from_numpy(p).to(dev) for p, _, _ in src], [torch.from_numpy(b).to(dev) for _, b, _ in src],
                                [torch.from_numpy(l).to(dev) for _, _, l in src], CLASSES)
    scenes = [scene(rng, a.points, int(rng.integers(5, 21))) for _ in range(a.scenes)]
    sample = dp.OBJECT_AUG.build(dict(type="ObjectSample", db_sampler=DB_SAMPLER), gt_database=db)
    noise = dp.OBJECT_AUG.build(NOISE)

    def fresh():
        return dp.pack_batch([torch.from_numpy(p).to(dev) for p, _, _ in scenes], [torch.from_numpy(b).to(dev) for _, b, _ in scenes],
                             "LiDAR", gt_labels_3d=[torch.from_numpy(l).to(dev) for _, _, l in scenes])

    for _ in range(3):
        noise(sample(fresh()))
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.iters):
        b = fresh()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b = noise(sample(b))
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    # the host restatement on the last batch's draws
    pts_h, off, lab_h = db.points.cpu().numpy(), db.obj_off_host, db.labels.cpu().numpy()
    host = []
    for _ in range(a.host_iters):
        t0 = time.perf_counter()
        for s, ((p, g, l), (rows, grp)) in enumerate(zip(scenes, b["db_sampled"])):
            w = R.paste_scene(p.astype(np.float64), g.astype(np.float64), l, db.boxes_host[rows], lab_h[rows],
                              [pts_h[off[r]:off[r + 1]] for r in rows], grp, True)
            R.object_noise(w["boxes"], w["points"], b["object_noise"]["loc"][s].astype(np.float64),
                           b["object_noise"]["rot"][s].astype(np.float64))
        host.append((time.perf_counter() - t0) * 1e3)
    so, go = b["scene_off"].tolist(), b["gt_off"].tolist()
    print(json.dumps(dict(metric="objaug_ms_per_batch", scenes=a.scenes, raw_points=a.points, db_objects=len(db),
                          candidates=int(sum(len(r) for r, _ in b["db_sampled"])), accepted=int(b["db_accepted"].sum()),
                          out_points=so[-1], out_boxes=go[-1], device_ms_median=float(np.median(ms)), device_ms_min=float(np.min(ms)),
                          host_ms_median=float(np.median(host)))))


if __name__ == "__main__":
    main()
