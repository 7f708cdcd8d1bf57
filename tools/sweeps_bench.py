"""Device time of the nuScenes sweep merge + PointsRangeFilter + PointShuffle on a batch of nuScenes-shaped samples against the NumPy
host restatement of LoadPointsFromMultiSweeps (tests/sweeps_ref.py, the per-sample work upstream runs in DataLoader workers), on the
same choices.  The host-to-device upload of the raw sweep rows (pack_batch(..., sweeps=...)) is timed on its own.

    python tools/sweeps_bench.py [--scenes 4] [--rows 34720] [--sweeps 9] [--iters 10]

Prints one JSON line: device ms per batch (median of --iters, events around the three transforms together and around each one),
upload ms per batch (wall clock around pack_batch, synchronised), host ms per sample and the row counts behind them.  The sweep files
are written to a temporary directory first; file reads are not timed on either side."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import sweeps_ref as R  # noqa: E402
from uni3detr_amd import datapath as dp  # noqa: E402

ENTRY = dict(type="LoadPointsFromMultiSweeps", sweeps_num=9, use_dim=[0, 1, 2, 3, 4], pad_empty_sweeps=True, remove_close=True)
PC_RANGE = [-54, -54, -5.0, 54, 54, 3.0]


def frame(rng, n):
    r = rng.uniform(0.5, 70, n)
    a = rng.uniform(-np.pi, np.pi, n)
    return np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-3, 2, n), rng.uniform(0, 255, n), np.zeros(n)], 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--rows", type=int, default=34720)
    ap.add_argument("--sweeps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sweeps_bench measures the device path: it needs the GPU"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    np.random.seed(0)
    tmp = tempfile.mkdtemp(prefix="sweeps_bench_")
    keys, infos = [], []
    for s in range(a.scenes):
        keys.append(frame(rng, a.rows))
        sw = []
        for j in range(a.sweeps + 1):
            path = os.path.join(tmp, f"s{s}_{j}.bin")
            frame(rng, a.rows + int(rng.integers(-500, 500))).tofile(path)
            c, si = np.cos(0.01 * j), np.sin(0.01 * j)
            sw.append(dict(data_path=path, timestamp=1_533_151_603_547_000 - 50_000 * (j + 1),
                           sensor2lidar_rotation=np.array([[c, -si, 0], [si, c, 0], [0, 0, 1]]),
                           sensor2lidar_translation=np.array([0.5 * j, 0.1 * j, 0.01])))
        infos.append(dict(timestamp=1_533_151_603.547, sweeps=sw))
    recs = [dp.read_sweeps(i, ENTRY) for i in infos]
    merge = dp.OBJECT_AUG.build(ENTRY)
    rf = dp.PointsRangeFilter(PC_RANGE)
    shuffle = dp.OBJECT_AUG.build(dict(type="PointShuffle"))
    key_d = [torch.from_numpy(k).to(dev) for k in keys]

    def fresh():
        return dp.pack_batch(key_d, box_type_3d="LiDAR", sweeps=recs)

    for _ in range(3):
        shuffle(rf(merge(fresh())))
    torch.cuda.synchronize()
    ms, up = [], []
    for _ in range(a.iters):
        t0 = time.perf_counter()
        b = fresh()
        torch.cuda.synchronize()
        up.append((time.perf_counter() - t0) * 1e3)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        b = merge(b)
        ev[1].record()
        b = rf(b)
        ev[2].record()
        b = shuffle(b)
        ev[3].record()
        torch.cuda.synchronize()
        ms.append([ev[0].elapsed_time(ev[3])] + [ev[k].elapsed_time(ev[k + 1]) for k in range(3)])
    ms = np.asarray(ms)
    host = []
    for k, info, rec in zip(keys, infos, recs):
        pts = [p.copy() for p in rec["points"]]
        t0 = time.perf_counter()
        R.load_points_from_multi_sweeps(k, info["sweeps"], info["timestamp"], 9, 5, [0, 1, 2, 3, 4], True, True, choices=rec["choices"],
                                        read=lambda path, it=iter(pts): next(it).reshape(-1))
        host.append((time.perf_counter() - t0) * 1e3)
    raw_rows = sum(sum(len(p) for p in r["points"]) for r in recs)
    so = b["scene_off"].tolist()
    print(json.dumps(dict(metric="sweeps_ms_per_batch", scenes=a.scenes, key_rows=a.rows, sweeps=a.sweeps, raw_sweep_rows=raw_rows,
                          merged_rows=so[-1], live_rows=int(b["count"].sum()), device_ms_median=float(np.median(ms[:, 0])),
                          device_ms_min=float(np.min(ms[:, 0])), merge_ms_median=float(np.median(ms[:, 1])),
                          range_filter_ms_median=float(np.median(ms[:, 2])), shuffle_ms_median=float(np.median(ms[:, 3])),
                          upload_ms_median=float(np.median(up)),
                          host_ms_per_sample_median=float(np.median(host)))))


if __name__ == "__main__":
    main()
