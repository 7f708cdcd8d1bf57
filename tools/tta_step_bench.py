"""Test-time augmentation behind the batched tail, timed two ways (GPU box; not part of bench.py).

(a) The multi-view merge alone: u3d_tta_merge_padded (padded rows, device counts, static grids) against u3d_tta_merge (ragged rows,
    host-known offsets and row count) on the same synthetic detections, both called through the C ABI on preallocated buffers, so
    neither pays native.tta_merge's host preparation.  Shapes, 2 samples x 4 views (double flip): 4 x 150 rows and 3 classes (KITTI),
    4 x 500 and 10 classes (nuScenes after num_thr = 500), and 4 x 900 (nuScenes' coder max_num, the largest views x K a shipped config
    with the double-flip block gives): above U3D_TTA_LDS_CAP the padded entry always launches the mask / sweep pair on a grid of
    views x K rows, whatever the counts are.  The 4 x 900 shape is therefore timed with 500 live rows per view - the ragged entry then
    sees 2000 candidates per sample and stays on the LDS path, so the difference is the static grid - and with all 900 live (both on
    the global path).  Device events around `calls` back-to-back calls.
(b) Dataset inference at a KITTI-shaped set - 64 samples in batches of 2 samples x 4 views - with the SUN RGB-D model (bf16, folded):
    per batch eager InferenceModel.aug_test + IndoorEvaluator.add() against InferenceStep(views=4) + testing.test_dataset + DetStore +
    add_store().  Files in a temporary directory, a BatchFeeder whose pipeline carries the MultiScaleFlipAug3D block (it yields the
    expanded dicts as they are), both loops seeded per batch, alternating inside one process, every round ending in a synchronise.

    python tools/tta_step_bench.py [--samples 64] [--batch 2] [--points 16000] [--rounds 10] [--warmup 2] [--calls 50] [--out FILE]

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
from uni3detr_amd import native as nv  # noqa: E402
from uni3detr_amd import testing, tta  # noqa: E402
from uni3detr_amd.configs.sunrgbd import model as MODEL_CFG  # noqa: E402
from uni3detr_amd.det_store import DetStore  # noqa: E402
from uni3detr_amd.feeder import BatchFeeder  # noqa: E402
from uni3detr_amd.inference import InferenceModel, InferenceStep  # noqa: E402
from uni3detr_amd.registry import build_model  # noqa: E402
from uni3detr_amd.synth import room_scene  # noqa: E402

SEED = 77
RANGE = [-3.2, -0.2, -2.0, 3.2, 6.2, 0.56]
INNER = [dict(type="GlobalRotScaleTrans", rot_range=[0, 0], scale_ratio_range=[1.0, 1.0], translation_std=[0, 0, 0]),
         dict(type="RandomFlip3D"), dict(type="PointsRangeFilter", point_cloud_range=RANGE)]
PIPELINE = [dict(dp.SHIPPED_LOAD_ENTRIES["sunrgbd"]),
            dict(type="MultiScaleFlipAug3D", img_scale=(1333, 800), pts_scale_ratio=1, flip=True, pcd_horizontal_flip=True,
                 pcd_vertical_flip=True, transforms=INNER)]
A = 4


def stats(xs, nd=3):
    return dict(median=round(statistics.median(xs), nd), min=round(min(xs), nd), max=round(max(xs), nd))


def events(fn, calls, reps, warmup):
    """ms per call: device events around `calls` back-to-back calls, `reps` samples after `warmup`"""
    out = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        if r >= warmup:
            out.append(e0.elapsed_time(e1) / calls)
    return out


def merge_case(dev, name, K, ncls, live, calls, reps, warmup, B=2, dim=7, max_num=500):
    """one shape of (a): B samples x A views, K padded rows of which `live` per view carry a detection"""
    rng = np.random.default_rng(K + live)
    V = B * A
    boxes = np.concatenate([rng.uniform(-50, 50, (V, K, 2)), rng.uniform(-2, 0, (V, K, 1)), rng.uniform(1.0, 4.5, (V, K, 3)),
                            rng.uniform(-3.1, 3.1, (V, K, 1))], 2).astype(np.float32)
    scores = rng.uniform(0.05, 1.0, (V, K)).astype(np.float32)
    labels = rng.integers(0, ncls, (V, K)).astype(np.int32)
    t = lambda a: torch.from_numpy(a).to(dev)                                          # noqa: E731
    det = nv.DetBatch(t(boxes), t(scores), t(labels), torch.full((V,), live, dtype=torch.int32, device=dev), None)
    metas = [dict(rot_degree=0.0, pcd_scale_factor=1.0, pcd_horizontal_flip=h, pcd_vertical_flip=v) for h in (False, True) for v in (False, True)]
    tab = tta.view_params(metas * B, dev)
    out = nv.tta_merge_padded(det, tab, A, tta.LIDAR, ncls, max_num=max_num)
    padded = lambda: nv.tta_merge_padded(det, tab, A, tta.LIDAR, ncls, max_num=max_num, out=out)            # noqa: E731
    # the ragged entry on the compacted rows, straight through the C ABI on preallocated buffers
    n = V * live
    rb, rs, rl = (x[:, :live].reshape((n,) + x.shape[2:]).contiguous() for x in (det.boxes, det.scores, det.labels))
    off = torch.arange(0, n + 1, live, dtype=torch.int32, device=dev)
    per_scene = A * live
    wsb = int(nv.lib().u3d_tta_merge_workspace(n, dim, B, A, ncls, per_scene))
    ws = torch.empty((max(wsb, 1),), dtype=torch.uint8, device=dev)
    ob, os_, ol, oc = (torch.empty((B, max_num, dim), device=dev), torch.empty((B, max_num), device=dev),
                       torch.empty((B, max_num), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev))
    p = nv._ptr

    def ragged():
        rc = nv.lib().u3d_tta_merge(p(rb), p(rs), p(rl), n, dim, p(off), p(tab), B, A, tta.LIDAR, ncls, 0.1, max_num, per_scene, p(ws), wsb,
                                    p(ob), p(os_), p(ol), p(oc), nv._stream())
        assert rc == 0, rc
    ragged()
    padded()
    cnt = out.count.tolist()
    same = out.count.tolist() == oc.tolist() and all(torch.equal(out.boxes[b, :c], ob[b, :c]) and torch.equal(out.scores[b, :c], os_[b, :c])
                                                     for b, c in enumerate(cnt))
    return dict(shape=name, samples=B, views=A, K=K, live_rows_per_view=live, classes=ncls, candidates_per_sample=per_scene,
                padded_global_path=A * K > nv.TTA_LDS_CAP, ragged_global_path=per_scene > nv.TTA_LDS_CAP, merged_per_sample=cnt,
                identical=bool(same), padded_ms=stats(events(padded, calls, reps, warmup), 4), ragged_ms=stats(events(ragged, calls, reps, warmup), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--points", type=int, default=16000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tta_step_bench measures the device path: it needs the GPU"
    assert a.samples % a.batch == 0 and a.rounds >= 1
    dev = torch.device("cuda:0")
    B, nb = a.batch, a.samples // a.batch

    # ---- (a) the merge alone --------------------------------------------------------------------------------------------------------
    reps = max(a.rounds, 10)
    merges = [merge_case(dev, "KITTI 4 x 150", 150, 3, 150, a.calls, reps, a.warmup),
              merge_case(dev, "nuScenes 4 x 500", 500, 10, 500, a.calls, reps, a.warmup),
              merge_case(dev, "nuScenes 4 x 900, 500 live", 900, 10, 500, a.calls, reps, a.warmup),
              merge_case(dev, "nuScenes 4 x 900, all live", 900, 10, 900, a.calls, reps, a.warmup)]
    assert all(m["identical"] for m in merges), "the padded entry must give the ragged entry's bytes"

    # ---- (b) the dataset loop -------------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(0)
    tmp = tempfile.mkdtemp(prefix="tta_step_bench_")
    try:
        samples, gts, labs = [], [], []
        for k in range(a.samples):
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
        inf = InferenceModel(model)
        step = InferenceStep(inf, batch_size=B, point_capacity=a.points, views=A)
        first = sync_batch(0)
        assert first["tta_views"] == A and tuple(first["tta_params"].shape) == (B * A, 9) and first["scene_off"].numel() == B * A + 1
        step.capture(batches=[first] + [sync_batch(i) for i in range(1, nb)], margin=1.25, warmup=3)
        store = DetStore(a.samples, step.tta_max_num, 7, dev)
        seed = lambda i: torch.manual_seed(SEED + i)                                    # noqa: E731

        def feeder():
            return BatchFeeder(samples, range(a.samples), dp.DevicePipeline(PIPELINE, load=True), batch_size=B, device=dev, drop_last=False)

        def loop_eager():
            e = ev.IndoorEvaluator(num_classes, device=dev)
            with feeder() as f:
                for i, batch in enumerate(f):
                    seed(i)
                    points, metas = dp.tta_forward_inputs(batch)
                    e.add(inf.aug_test(points, metas), gts[i * B:(i + 1) * B], labs[i * B:(i + 1) * B])
            return e.compute()

        def loop_store():
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
            ra, rb = loop_eager(), loop_store()
        identical = set(ra) == set(rb) and all(np.float64(ra[k]).tobytes() == np.float64(rb[k]).tobytes() for k in ra)
        fallbacks0 = step.fallbacks
        ms = dict(a=[], b=[])
        for _ in range(a.rounds):                               # alternating: both see the same machine
            ms["a"].append(timed(loop_eager)[0])
            ms["b"].append(timed(loop_store)[0])
        out = dict(metric="tta_step_ab", merge=merges, samples=a.samples, batch=B, views=A, points=a.points, rounds=a.rounds, warmup=a.warmup,
                   eager_loop_ms=dict(whole_set=stats(ms["a"]), per_batch=stats([x / nb for x in ms["a"]])),
                   store_loop_ms=dict(whole_set=stats(ms["b"]), per_batch=stats([x / nb for x in ms["b"]])),
                   detections=int(store.cursor[1]), fallbacks_in_timed_rounds=step.fallbacks - fallbacks0, metrics_identical=bool(identical),
                   mAP_025=ra.get("mAP_0.25"))
        da, db = out["eager_loop_ms"]["whole_set"], out["store_loop_ms"]["whole_set"]
        lines = ["(a) The multi-view merge alone, 2 samples x 4 views (MI355X): ms per call, medians (min .. max) of "
                 f"{reps} samples of {a.calls} back-to-back calls after {a.warmup} warm-up samples; device events; C ABI calls on preallocated buffers."]
        for m in merges:
            pm, rm = m["padded_ms"], m["ragged_ms"]
            lines.append(f"  {m['shape']:<28} {m['candidates_per_sample']:5d} candidates/sample  padded {pm['median']:.4f} ({pm['min']:.4f} .. {pm['max']:.4f})"
                         f"{' [mask/sweep grid]' if m['padded_global_path'] else ''}   ragged {rm['median']:.4f} ({rm['min']:.4f} .. {rm['max']:.4f})"
                         f"{' [mask/sweep grid]' if m['ragged_global_path'] else ''}   padded - ragged {pm['median'] - rm['median']:+.4f}   identical: {m['identical']}")
        lines += [
            f"(b) Dataset inference with double-flip TTA over {a.samples} samples x {a.points} points, B = {B} samples x {A} views, SUN RGB-D model, "
            f"bf16 folded, BatchFeeder with the MultiScaleFlipAug3D block (MI355X).",
            f"Medians of {a.rounds} alternating rounds after {a.warmup} warm-up rounds (min .. max); each round ends in a device synchronise.",
            f"  eager inf.aug_test() + IndoorEvaluator.add() per batch, compute():           {da['median']:9.3f} ms  ({da['min']:.3f} .. {da['max']:.3f})"
            f"   = {da['median'] / nb:.3f} ms per batch",
            f"  InferenceStep(views={A}) + test_dataset + DetStore, add_store(), compute():     {db['median']:9.3f} ms  ({db['min']:.3f} .. {db['max']:.3f})"
            f"   = {db['median'] / nb:.3f} ms per batch",
            f"  metric dicts identical: {identical}; eager fallbacks in the timed rounds: {out['fallbacks_in_timed_rounds']}",
            ("  the captured loop is faster than the eager one beyond the eager loop's measured spread." if db["median"] < da["min"] else
             "  the captured loop is NOT faster than the eager one beyond its measured spread: what it removes is the per-batch host read."),
            json.dumps(out),
        ]
        text = "\n".join(lines) + "\n"
        print(text, end="", flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(text)
        assert identical, "the two loops must give the same metric dict when both are seeded per batch"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
