"""Indoor evaluation timing on synthetic val-shaped sets: the device path (csrc/eval.hip) over the whole set, the float64 host path on a
subset.  Prints one JSON line.

  timeout -k 10 600 python tools/eval_bench.py [--sets sunrgbd,scannet] [--host-scenes 100]

SUN RGB-D val: 5050 scenes x 1000 detections, 10 classes; ScanNet val: 312 scenes x 5000 detections, 18 classes (the shipped configs'
max_num).  Device ms: event-timed end-to-end `indoor_eval` core (validation, kernels, sort, result copy) on device-resident inputs,
median of 5 after 2 warm-up runs.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uni3detr_amd import evaluation as ev  # noqa: E402
from uni3detr_amd.eval_common import offsets  # noqa: E402
from uni3detr_amd.synth import eval_scenes  # noqa: E402

SETS = {"sunrgbd": (5050, 1000, 10, 12), "scannet": (312, 5000, 18, 40)}


def flat(data):
    return (np.concatenate([d[2] for d in data]), np.concatenate([d[3] for d in data]), np.concatenate([d[4] for d in data]),
            np.array([len(d[4]) for d in data]), np.concatenate([ev._gt_bottom_boxes(d[0]) for d in data]),
            np.concatenate([d[1] for d in data]), np.array([len(d[1]) for d in data]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="sunrgbd,scannet")
    ap.add_argument("--host-scenes", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"workload": "indoor_eval"}
    for name in a.sets.split(","):
        n_scenes, n_det, ncls, max_gt = SETS[name]
        data = eval_scenes(n_scenes, n_det, ncls, seed=0, max_gt=max_gt)
        db, ds, dl, dc, gb, gl, gc = flat(data)
        f32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)                          # noqa: E731
        i32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.int32)).to(dev)                            # noqa: E731
        args = (f32(db), f32(ds), i32(dl), i32(offsets(dc)), f32(gb), i32(gl), i32(offsets(gc)), ncls, (0.25, 0.5), dev)
        times = []
        for r in range(2 + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            res = ev._device_eval(*args)
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                times.append(e0.elapsed_time(e1))
        hs = min(a.host_scenes, n_scenes)
        hdb, hds, hdl, hdc, hgb, hgl, hgc = flat(data[:hs])
        t0 = time.perf_counter()
        ev.evaluate_flat(hdb, hds, hdl, hdc, hgb, hgl, hgc, ncls, (0.25, 0.5), "cpu")
        host_ms = (time.perf_counter() - t0) * 1e3
        out[name] = {"scenes": n_scenes, "detections": int(len(dl)), "gt": int(len(gl)), "classes": ncls,
                     "device_ms_median": round(statistics.median(times), 3), "device_ms_min": round(min(times), 3),
                     "host_ms": round(host_ms, 1), "host_scenes": hs,
                     "mAP_0.25": float(np.nanmean(np.where(res["npos"] > 0, res["ap"][0], np.nan)))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
