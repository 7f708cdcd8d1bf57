"""What watching the loss costs a captured training loop, at the benched SUN RGB-D size (GPU box; not part of bench.py).

B = 8 scenes of 20 000 points, bf16, the captured TrainStep of bench.py, `--batches` rotating synthetic batches.  Three loops of
`--steps` steps each, alternating `--reps` times in one process, host clock around each loop, every loop ending in a device synchronise:
  (a) bare replay: set_batch + step(), nothing read (what a loop could do before the step log);
  (b) the same with TrainStep(log=StepLog()) - one u3d_step_log_append inside the last captured stage - and log.window(50) every 50 steps;
  (c) (a) with ts.loss.item() after every step (the only way to see a loss without the log).
(a) / (c) and (b) are two TrainStep objects over two models built from the same seed: the log changes what is captured.

    python tools/train_loop_bench.py [--steps 100] [--reps 3] [--warmup 10] [--batches 8] [--out FILE]

The claim to check is (b) against (a): the log may cost at most the run-to-run spread of (a), min to max over the repetitions.
Prints the report and one JSON line, and writes both to --out."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import projects.mmdet3d_plugin  # noqa: E402,F401
from bench import WORKLOADS, make_batch, workload_cfg  # noqa: E402
from uni3detr_amd.registry import build_model  # noqa: E402
from uni3detr_amd.step_log import StepLog  # noqa: E402
from uni3detr_amd.trainer import TrainStep  # noqa: E402


def build(dev, rot, cfg, log):
    torch.manual_seed(1234)
    model = build_model(cfg).to(dev).train()
    model.set_precision("bf16")
    d = rot[0]
    ts = TrainStep(model, d["points"], d["gt_bboxes_3d"], d["gt_labels_3d"], graph=True, overlap_reduce=True, log=log)
    ts.capture(batches=[(d["points"], d["gt_bboxes_3d"], d["gt_labels_3d"]) for d in rot])
    packed = [(model.pack_points(d["points"]), model.pts_bbox_head.pack_gts(d["gt_bboxes_3d"], d["gt_labels_3d"], dev), None) for d in rot]
    return ts, packed


def loop(ts, packed, steps, after=None):
    """ms per step of `steps` steps, host clock, ending in a device synchronise; after(i): the host's look at the loss"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        ts.set_batch(*packed[i % len(packed)])
        ts.step()
        if after is not None:
            after(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "train_loop_bench.py needs an MI355X"
    dev = torch.device("cuda", 0)
    wl, cfg = WORKLOADS["sunrgbd"], workload_cfg("sunrgbd")
    rot = [make_batch(0, wl["batch"], wl["points"], dev, index=j, cfg=cfg) for j in range(a.batches)]
    bare, bare_packed = build(dev, rot, cfg, None)
    log = StepLog(device=dev)
    logged, logged_packed = build(dev, rot, cfg, log)
    seen = []

    def window(i):
        if (i + 1) % 50 == 0:
            seen.append(log.window(50)["loss"])

    def item(i):
        seen.append(bare.loss.item())

    sides = dict(a=lambda n: loop(bare, bare_packed, n), b=lambda n: loop(logged, logged_packed, n, window),
                 c=lambda n: loop(bare, bare_packed, n, item))
    for fn in sides.values():                      # warm-up: every side once, short
        fn(a.warmup)
    ms = {k: [] for k in sides}
    for _ in range(a.reps):
        for k, fn in sides.items():
            ms[k].append(fn(a.steps))
    stat = {k: dict(min=round(min(v), 4), max=round(max(v), 4), all=[round(x, 4) for x in v]) for k, v in ms.items()}
    spread = stat["a"]["max"] - stat["a"]["min"]
    extra = min(ms["b"]) - min(ms["a"]), max(ms["b"]) - max(ms["a"])
    within = extra[0] <= spread and extra[1] <= spread
    out = dict(metric="train_loop_ab", batch=wl["batch"], points=wl["points"], steps=a.steps, reps=a.reps, rotating_batches=a.batches,
               ms_per_step=stat, spread_a_ms=round(spread, 4), log_rows=len(log), log_within_spread_of_a=bool(within))
    lines = [
        f"Captured SUN RGB-D training step, B = {wl['batch']} x {wl['points']} points, bf16 (ms per step, host clock over {a.steps} steps ending "
        f"in a device synchronise, {a.reps} alternating repetitions, min .. max):",
        f"  (a) bare replay:                                        {stat['a']['min']:.4f} .. {stat['a']['max']:.4f}   {stat['a']['all']}",
        f"  (b) replay + step log, log.window(50) every 50 steps:   {stat['b']['min']:.4f} .. {stat['b']['max']:.4f}   {stat['b']['all']}",
        f"  (c) replay + ts.loss.item() every step:                 {stat['c']['min']:.4f} .. {stat['c']['max']:.4f}   {stat['c']['all']}",
        f"  run-to-run spread of (a): {spread:.4f} ms; (b) - (a): {extra[0]:+.4f} ms (min against min), {extra[1]:+.4f} ms (max against max)",
        "  the log costs " + ("no more than" if within else "MORE than") + " the run-to-run spread of (a).",
        "", json.dumps(out)]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
