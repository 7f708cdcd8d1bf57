"""KITTI evaluation timing on a KITTI-val-shaped set (3769 scenes, up to 150 detections each, synth.kitti_scenes).

Device: the whole evaluation from records already on the device (overlaps, flags, both passes, thresholds, AP; host synchronisations
included), the median of --runs after --warmup, and KittiEvaluator.compute() (LiDAR conversion included) the same way.
Host: the float64 NumPy path on the first --host-scenes scenes; the full-set figure is that time scaled by the scene count and is
printed as an extrapolation.  One JSON line at the end.
    python tools/kitti_eval_bench.py [--scenes 3769] [--max-det 150] [--runs 10] [--host-scenes 100]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uni3detr_amd import kitti_eval as ke  # noqa: E402
from uni3detr_amd.synth import kitti_scenes  # noqa: E402

CLASSES = ["Pedestrian", "Cyclist", "Car"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=3769)
    ap.add_argument("--max-det", type=int, default=150)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-scenes", type=int, default=100)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark times the MI355X"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    t0 = time.perf_counter()
    infos, results = kitti_scenes(a.scenes, det_per_scene=rng.integers(a.max_det // 2, a.max_det + 1, a.scenes), seed=0)
    gt_annos = [i["annos"] for i in infos]
    dt_annos = ke.lidar_results_to_kitti(results, infos, CLASSES)
    gen_s = time.perf_counter() - t0
    class_ids, metrics = ke._class_ids(CLASSES), [0, 1, 2]
    gt, gc = ke._encode_all(gt_annos, True)
    dt, dc = ke._encode_all(dt_annos, False)
    aos = ke._compute_aos(gt_annos, dt_annos)
    d, doff = ke._upload(dt, dc, dev)
    g, goff = ke._upload(gt, gc, dev)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ts = []
        for _ in range(a.runs):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) * 1e3)
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

    core = timed(lambda: ke._device_core(d, doff, g, goff, dc, gc, class_ids, metrics, aos))
    ev = ke.KittiEvaluator(CLASSES, device=dev)
    ev.add(results, infos)
    evaluator = timed(ev.compute)
    # host path on a subset
    k = min(a.host_scenes, a.scenes)
    t = time.perf_counter()
    ke.host_core(dt[:int(np.sum(dc[:k]))], dc[:k], gt[:int(np.sum(gc[:k]))], gc[:k], class_ids, metrics, aos)
    host_s = time.perf_counter() - t
    n_det, n_gt = int(np.sum(dc)), int(np.sum(gc))
    print(f"[kitti_eval_bench] {a.scenes} scenes, {n_det} valid detections, {n_gt} GT rows (set built in {gen_s:.1f} s)")
    print(f"  device core       median {core[0]:.2f} ms (min {core[1]:.2f}, max {core[2]:.2f}) over {a.runs} runs")
    print(f"  KittiEvaluator    median {evaluator[0]:.2f} ms (min {evaluator[1]:.2f}, max {evaluator[2]:.2f})")
    print(f"  host path         {host_s:.2f} s for {k} scenes; extrapolated to {a.scenes} scenes: {host_s * a.scenes / k:.1f} s")
    print(json.dumps(dict(scenes=a.scenes, detections=n_det, gt=n_gt, device_core_ms=core[0], evaluator_ms=evaluator[0],
                          host_subset_scenes=k, host_subset_s=host_s, host_extrapolated_s=host_s * a.scenes / k)))


if __name__ == "__main__":
    main()
