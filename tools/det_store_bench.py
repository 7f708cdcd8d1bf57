"""Dataset inference two ways at the SUN RGB-D shape (GPU box; not part of bench.py): the per-batch host round trip against the
device-resident detection store (uni3detr_amd/det_store.py, uni3detr_amd/testing.py).

64 synthetic scenes of 20 000 points as .bin files in a temporary directory, B = 8, bf16, a BatchFeeder into a captured InferenceStep.
Two loops over the same files, alternating inside one process, every round ending in a device synchronise:
  (a) per batch step.results() (five device-to-host copies and a synchronisation) + IndoorEvaluator.add(), then compute();
  (b) testing.test_dataset (step.run + DetStore.append, no host read per batch) + IndoorEvaluator.add_store(), then compute().
Both seed the generator per batch (the head draws random query points), and the two metric dicts are asserted identical once.
u3d_det_store_append alone is timed with device events on the step's own DetBatch.

    python tools/det_store_bench.py [--scenes 64] [--batch 8] [--points 20000] [--rounds 20] [--warmup 3] [--out FILE]

Prints the report (medians with min .. max, and one JSON line) and writes it to --out."""
import argparse
import copy
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import projects.mmdet3d_plugin  # noqa: E402,F401
from oracle.weights import seeded_tensor  # noqa: E402
from uni3detr_amd import datapath as dp  # noqa: E402
from uni3detr_amd import evaluation as ev  # noqa: E402
from uni3detr_amd import testing  # noqa: E402
from uni3detr_amd.configs.sunrgbd import model as MODEL_CFG  # noqa: E402
from uni3detr_amd.det_store import DetStore  # noqa: E402
from uni3detr_amd.feeder import BatchFeeder  # noqa: E402
from uni3detr_amd.inference import InferenceModel, InferenceStep  # noqa: E402
from uni3detr_amd.registry import build_model  # noqa: E402
from uni3detr_amd.synth import room_scene  # noqa: E402

SEED = 77
PIPELINE = [dict(dp.SHIPPED_LOAD_ENTRIES["sunrgbd"]), dict(type="PointsRangeFilter", point_cloud_range=[-3.2, -0.2, -2.0, 3.2, 6.2, 0.56]),
            dict(type="DefaultFormatBundle3D"), dict(type="Collect3D")]


def stats(xs):
    return dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=64)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "det_store_bench measures the device path: it needs the GPU"
    assert a.scenes % a.batch == 0 and a.rounds >= 1
    dev = torch.device("cuda:0")
    B, nb = a.batch, a.scenes // a.batch
    rng = np.random.default_rng(0)
    tmp = tempfile.mkdtemp(prefix="det_store_bench_")
    try:
        samples, gts, labs = [], [], []
        for k in range(a.scenes):
            p, g, l = room_scene(k, a.points)
            path = os.path.join(tmp, f"scan{k}.bin")
            np.concatenate([p[:, :3], rng.integers(0, 256, (a.points, 3)).astype(np.float32)], 1).tofile(path)
            samples.append(dict(pts_filename=path))
            gts.append(torch.from_numpy(g).to(dev))
            labs.append(torch.from_numpy(l % 10).to(dev))
        pipe = dp.DevicePipeline(PIPELINE, load=True)

        def sync_batch(i):
            recs = [dp.read_points(samples[k], pipe.load_cfg) for k in range(i * B, (i + 1) * B)]
            return pipe(dp.pack_batch(None, raw=recs, device=dev))

        model = build_model(copy.deepcopy(MODEL_CFG))
        model.load_state_dict({k: seeded_tensor(k, tuple(v.shape), 3) for k, v in model.state_dict().items()})
        model = model.to(dev).set_precision("bf16").eval()
        num_classes = int(model.pts_bbox_head.num_classes)
        step = InferenceStep(InferenceModel(model), batch_size=B, point_capacity=a.points)
        step.capture(batches=[sync_batch(i) for i in range(nb)], margin=1.25, warmup=3)
        K = int(step.det.boxes.shape[1])
        store = DetStore(a.scenes, K, 7, dev)
        seed = lambda i: torch.manual_seed(SEED + i)                                    # noqa: E731

        def feeder():
            return BatchFeeder(samples, range(a.scenes), dp.DevicePipeline(PIPELINE, load=True), batch_size=B, device=dev, drop_last=False)

        def loop_a():
            e = ev.IndoorEvaluator(num_classes, device=dev)
            with feeder() as f:
                for i, batch in enumerate(f):
                    seed(i)
                    e.add(step.results(batch), gts[i * B:(i + 1) * B], labs[i * B:(i + 1) * B])
            return e.compute()

        def loop_b():
            store.reset()
            e = ev.IndoorEvaluator(num_classes, device=dev)
            with feeder() as f:
                testing.test_dataset(step, f, store, reload=lambda i: sync_batch(i), on_batch=seed)
            e.add_store(store, gts, labs)
            return e.compute()

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out

        for _ in range(a.warmup):
            ra, rb = loop_a(), loop_b()
        identical = set(ra) == set(rb) and all(np.float64(ra[k]).tobytes() == np.float64(rb[k]).tobytes() for k in ra)
        assert identical, "the two loops must give the same metric dict"
        fallbacks0 = step.fallbacks
        ms = dict(a=[], b=[])
        for _ in range(a.rounds):                               # alternating: both see the same machine
            ms["a"].append(timed(loop_a)[0])
            ms["b"].append(timed(loop_b)[0])

        # u3d_det_store_append alone, on the DetBatch the last replay left
        alone = DetStore(B * 64, K, 7, dev)
        ap_ms = []
        for r in range(a.warmup + max(a.rounds, 20)):
            alone.reset()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(64):
                alone.append(step.det, n_live=step.n_live, valid=step.valid)
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                ap_ms.append(e0.elapsed_time(e1) / 64)
        rows = int(alone.cursor[1]) // 64

        out = dict(metric="det_store_ab", scenes=a.scenes, batch=B, points=a.points, max_num=K, rounds=a.rounds, warmup=a.warmup,
                   per_batch_host_loop_ms=dict(whole_set=stats(ms["a"]), per_batch=stats([x / nb for x in ms["a"]])),
                   store_loop_ms=dict(whole_set=stats(ms["b"]), per_batch=stats([x / nb for x in ms["b"]])),
                   append_alone_ms=dict(stats(ap_ms), rows_per_call=rows, scenes_per_call=B, calls_per_sample=64),
                   detections=int(store.cursor[1]), fallbacks_in_timed_rounds=step.fallbacks - fallbacks0, metrics_identical=identical,
                   mAP_025=ra.get("mAP_0.25"))
        da, db = out["per_batch_host_loop_ms"]["whole_set"], out["store_loop_ms"]["whole_set"]
        faster = db["median"] < da["min"]
        lines = [
            f"Dataset inference over {a.scenes} scenes x {a.points} points, B = {B}, bf16, BatchFeeder -> captured InferenceStep (MI355X).",
            f"Medians of {a.rounds} alternating rounds after {a.warmup} warm-up rounds (min .. max); each round ends in a device synchronise.",
            f"  (a) step.results() + IndoorEvaluator.add() per batch, compute():   {da['median']:9.3f} ms  ({da['min']:.3f} .. {da['max']:.3f})"
            f"   = {da['median'] / nb:.3f} ms per batch",
            f"  (b) test_dataset + DetStore.append, add_store(), compute():        {db['median']:9.3f} ms  ({db['min']:.3f} .. {db['max']:.3f})"
            f"   = {db['median'] / nb:.3f} ms per batch",
            f"  u3d_det_store_append alone (device events, {B} scenes, {rows} rows per call, mean of 64 back-to-back calls): "
            f"{out['append_alone_ms']['median']:.4f} ms  ({out['append_alone_ms']['min']:.4f} .. {out['append_alone_ms']['max']:.4f})",
            f"  metric dicts identical: {identical}; eager fallbacks in the timed rounds: {out['fallbacks_in_timed_rounds']}",
            ("  (b) is faster than (a) beyond (a)'s measured spread." if faster else
             "  (b) is NOT faster than (a) beyond (a)'s measured spread: the step is device-bound, the store removes the per-batch host "
             "round trip from the interface, not time from the loop."),
            json.dumps(out),
        ]
        text = "\n".join(lines) + "\n"
        print(text, end="", flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(text)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
