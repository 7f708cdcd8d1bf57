"""nuScenes evaluation timing on a nuScenes-val-shaped set (6019 samples, 300-500 predictions and about 30 GT each, synth.nusc_samples).

Device: `nuscenes_eval(device=cuda)` end to end from host results (encoding and upload included) and `NuScenesEvaluator.compute()`
over everything already added (conversion, filters, matching, accumulation; host synchronisations included), each the median of --runs
after --warmup.  Host: the float64 NumPy path on the first --host-samples samples; the full-set figure is that time scaled by the
sample count and is printed as an extrapolation.  One JSON line at the end.
    python tools/nusc_eval_bench.py [--samples 6019] [--runs 5] [--host-samples 100]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uni3detr_amd import nuscenes_eval as ne  # noqa: E402
from uni3detr_amd.synth import nusc_samples  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=6019)
    ap.add_argument("--min-preds", type=int, default=300)
    ap.add_argument("--max-preds", type=int, default=500)
    ap.add_argument("--max-gt", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-samples", type=int, default=100)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark times the MI355X"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    t0 = time.perf_counter()
    infos, results = nusc_samples(a.samples, preds_per_sample=rng.integers(a.min_preds, a.max_preds + 1, a.samples), seed=0, max_gt=a.max_gt,
                                  miss=0.1, dup=0.3)
    gen_s = time.perf_counter() - t0

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

    full = timed(lambda: ne.nuscenes_eval(results, infos, device=dev, logger="silent"))
    ev = ne.NuScenesEvaluator(device=dev)
    ev.add(results, infos)
    evaluator = timed(ev.compute)
    k = min(a.host_samples, a.samples)
    t = time.perf_counter()
    host_k = ne.nuscenes_eval(results[:k], infos[:k], device="cpu", logger="silent")
    host_s = time.perf_counter() - t
    dev_k = ne.nuscenes_eval(results[:k], infos[:k], device=dev, logger="silent")
    worst = max(abs(dev_k[x] - host_k[x]) for x in host_k if not (np.isnan(host_k[x]) and np.isnan(dev_k[x])))
    n_pred = int(sum(len(r["scores_3d"]) for r in results))
    n_gt = int(sum(len(i["gt_names"]) for i in infos))
    print(f"[nusc_eval_bench] {a.samples} samples, {n_pred} predictions, {n_gt} GT rows (set built in {gen_s:.1f} s)")
    print(f"  nuscenes_eval (device)     median {full[0]:.1f} ms (min {full[1]:.1f}, max {full[2]:.1f}) over {a.runs} runs")
    print(f"  NuScenesEvaluator.compute  median {evaluator[0]:.1f} ms (min {evaluator[1]:.1f}, max {evaluator[2]:.1f})")
    print(f"  host path                  {host_s:.2f} s for {k} samples; extrapolated to {a.samples}: {host_s * a.samples / k:.0f} s; "
          f"device vs host on them: max |diff| {worst:.1e}")
    print(json.dumps(dict(samples=a.samples, predictions=n_pred, gt=n_gt, device_eval_ms=full[0], evaluator_ms=evaluator[0],
                          host_subset_samples=k, host_subset_s=host_s, host_extrapolated_s=host_s * a.samples / k, max_abs_diff_subset=worst)))


if __name__ == "__main__":
    main()
