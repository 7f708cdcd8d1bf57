"""Dynamic voxelization in the captured inference step at the ScanNet-large shape (GPU box; not part of bench.py).

B = 2 scenes of up to 150 000 points, 3 features (what the shipped loader keeps), the shipped grid (0.02 m voxels), bf16.

  Mean kernel   u3d_scatter_mean (f32 atomics; its caller's zeroing of sums and counts included, the contract demands it) against
                u3d_scatter_mean_exact (fixed-point integer atomics, zeroes for itself) on the same ranks, and the exact entry alone with
                every point in ONE voxel (the contention worst case).  Device events around `--calls` back-to-back calls, the two sides
                alternating.
  Step          InferenceStep replay against eager inf.simple_test_batched(..., on_device=True) on the same batch, alternating, device
                events; then a `--scenes`-scene set of differing sizes from .bin files through a BatchFeeder:
                (a) per batch step.results() + IndoorEvaluator.add(), compute();  (b) testing.test_dataset + DetStore, add_store(), compute().
                Host clock around each loop, ending in a device synchronise.  The two metric dicts are asserted identical once.

    python tools/dynvox_bench.py [--points 150000] [--batch 2] [--scenes 16] [--rounds 10] [--warmup 2] [--calls 20] [--out FILE]

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
from uni3detr_amd import testing  # noqa: E402
from uni3detr_amd.configs import variants  # noqa: E402
from uni3detr_amd.det_store import DetStore  # noqa: E402
from uni3detr_amd.feeder import BatchFeeder  # noqa: E402
from uni3detr_amd.inference import InferenceModel, InferenceStep  # noqa: E402
from uni3detr_amd.registry import build_model  # noqa: E402
from uni3detr_amd.synth import room_scene  # noqa: E402

SEED = 77
FEAT = 3


def stats(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4))


def fmt(s):
    return f"{s['median']:9.4f} ms  ({s['min']:.4f} .. {s['max']:.4f})"


def events(fn, calls):
    """ms per call of `calls` back-to-back calls between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def mean_kernels(a, dev, cfg, lines, out):
    vl = cfg["pts_voxel_layer"]
    pc = tuple(vl["point_cloud_range"])
    pts = [torch.from_numpy(np.ascontiguousarray(room_scene(k, a.points, pc_range=pc)[0][:, :FEAT])).to(dev) for k in range(a.batch)]
    cat = torch.cat(pts).contiguous()
    off = torch.tensor([a.points * k for k in range(a.batch + 1)], dtype=torch.int32, device=dev)
    coors = nv.voxelize_dynamic(cat, off, a.batch, vl["voxel_size"], vl["point_cloud_range"])
    dims = tuple(int(round((pc[3 + j] - pc[j]) / vl["voxel_size"][j])) for j in (2, 1, 0))
    g = nv.BitGrid(a.batch, dims, dev, linear=True)
    g.mark(coors)
    g.scan()
    n_vox = int(g.count_dev.item())
    rank = g.rank(coors)
    one = torch.zeros_like(rank)
    n = cat.shape[0]
    sums, counts = torch.empty((n_vox, FEAT), device=dev), torch.empty((n_vox,), dtype=torch.int32, device=dev)
    mean, cnt2 = torch.empty((n_vox, FEAT), device=dev), torch.empty((n_vox,), dtype=torch.int32, device=dev)
    wsb = int(nv.lib().u3d_scatter_mean_exact_workspace(n_vox, FEAT))
    ws = torch.empty(wsb // 8 + 1, dtype=torch.int64, device=dev)
    p, L = nv._ptr, nv.lib()

    def atomic():
        sums.zero_()
        counts.zero_()
        nv._check(L.u3d_scatter_mean(p(cat), p(rank), n, FEAT, p(sums), p(counts), n_vox, nv._stream()), "scatter_mean")

    def exact(r=rank):
        nv._check(L.u3d_scatter_mean_exact(p(cat), p(r), n, FEAT, p(mean), p(cnt2), n_vox, p(ws), ws.numel() * 8, nv._stream()), "scatter_mean_exact")

    sides = dict(atomic=atomic, exact=exact, exact_one_voxel=lambda: exact(one))
    ms = {k: [] for k in sides}
    for r in range(a.warmup + a.rounds):
        for k, fn in sides.items():                              # alternating: every side sees the same machine
            t = events(fn, a.calls)
            if r >= a.warmup:
                ms[k].append(t)
    atomic()
    exact()
    torch.cuda.synchronize()
    diff = float((sums - mean).abs().max())
    assert torch.equal(counts, cnt2)
    res = {k: stats(v) for k, v in ms.items()}
    out["mean_kernel_ms"] = dict(res, rows=n, voxels=n_vox, features=FEAT, calls_per_sample=a.calls, max_abs_difference=diff)
    lines += [
        f"Voxel mean, {n} rows x {FEAT} features into {n_vox} voxels (ms per call, device events over {a.calls} back-to-back calls,",
        f"medians of {a.rounds} alternating rounds after {a.warmup} warm-up rounds (min .. max)):",
        f"  u3d_scatter_mean (f32 atomics) + the caller's zeroing of sums and counts: {fmt(res['atomic'])}",
        f"  u3d_scatter_mean_exact (fixed point, order-free, zeroes for itself):      {fmt(res['exact'])}",
        f"  u3d_scatter_mean_exact, every row in ONE voxel (contention worst case):   {fmt(res['exact_one_voxel'])}",
        f"  largest |atomic mean - exact mean| on these points: {diff:.3e}; counts equal",
    ]


def step_and_dataset(a, dev, cfg, lines, out):
    pc = tuple(cfg["pts_voxel_layer"]["point_cloud_range"])
    B, nb = a.batch, a.scenes // a.batch
    rng = np.random.default_rng(0)
    tmp = tempfile.mkdtemp(prefix="dynvox_bench_")
    try:
        samples, gts, labs, sizes = [], [], [], []
        ncls = int(cfg["pts_bbox_head"]["num_classes"])
        for k in range(a.scenes):
            n = int(rng.integers(a.points * 2 // 3, a.points + 1)) if k else a.points      # test scenes differ in size; one is full
            pts, g, l = room_scene(k, n, pc_range=pc)
            path = os.path.join(tmp, f"scan{k}.bin")
            np.ascontiguousarray(pts[:, :FEAT], np.float32).tofile(path)
            samples.append(dict(pts_filename=path))
            gts.append(torch.from_numpy(g).to(dev))
            labs.append(torch.from_numpy(l % ncls).to(dev))
            sizes.append(n)
        pipeline = [dict(dp.SHIPPED_LOAD_ENTRIES["scannet_large"]), dict(type="PointsRangeFilter", point_cloud_range=list(pc)),
                    dict(type="DefaultFormatBundle3D"), dict(type="Collect3D")]
        pipe = dp.DevicePipeline(pipeline, load=True)

        def sync_batch(i):
            recs = [dp.read_points(samples[k], pipe.load_cfg) for k in range(i * B, (i + 1) * B)]
            return pipe(dp.pack_batch(None, raw=recs, device=dev))

        mcfg = copy.deepcopy(cfg)
        mcfg["pts_middle_encoder"]["in_channels"] = FEAT
        model = build_model(mcfg)
        model.load_state_dict({k: seeded_tensor(k, tuple(v.shape), 3) for k, v in model.state_dict().items()})
        model = model.to(dev).set_precision("bf16").eval()
        inf = InferenceModel(model)
        step = InferenceStep(inf, batch_size=B, point_capacity=a.points)
        counts, caps = step.capture(batches=[sync_batch(i) for i in range(nb)], margin=1.25, warmup=3)
        K = int(step.det.boxes.shape[1])
        seed = lambda i: torch.manual_seed(SEED + i)                                    # noqa: E731

        # ---- one batch: replay against the eager on-device path
        batch0 = sync_batch(0)
        scenes0 = list(dp.unpack_batch(batch0)[0])
        sides = dict(replay=lambda: step.run(batch0), eager=lambda: inf.simple_test_batched(None, scenes0, on_device=True))
        ms = {k: [] for k in sides}
        for r in range(a.warmup + a.rounds):
            for k, fn in sides.items():
                t = events(fn, max(a.calls // 4, 3))
                if r >= a.warmup:
                    ms[k].append(t)
        step.run(batch0)
        valid0 = int(step.valid)
        res = {k: stats(v) for k, v in ms.items()}
        out["step_ms_per_batch"] = dict(res, batch=B, rows=int(batch0["points"].shape[0]), voxel_capacity=caps[0], level_capacities=caps[1:],
                                        counts=counts, replay_valid=valid0)

        # ---- the set: per-batch host loop against the store loop
        store = DetStore(a.scenes, K, 7, dev)

        def feeder():
            return BatchFeeder(samples, range(a.scenes), dp.DevicePipeline(pipeline, load=True), batch_size=B, device=dev, drop_last=False)

        def loop_a():
            e = ev.IndoorEvaluator(ncls, device=dev)
            with feeder() as f:
                for i, batch in enumerate(f):
                    seed(i)
                    e.add(step.results(batch), gts[i * B:(i + 1) * B], labs[i * B:(i + 1) * B])
            return e.compute()

        def loop_b():
            store.reset()
            e = ev.IndoorEvaluator(ncls, device=dev)
            with feeder() as f:
                testing.test_dataset(step, f, store, reload=lambda i: sync_batch(i), on_batch=seed)
            e.add_store(store, gts, labs)
            return e.compute()

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, r

        for _ in range(max(a.warmup, 1)):
            ra, rb = loop_a(), loop_b()
        identical = set(ra) == set(rb) and all(np.float64(ra[k]).tobytes() == np.float64(rb[k]).tobytes() for k in ra)
        assert identical, "the two loops must give the same metric dict"
        fb0 = step.fallbacks
        sets = dict(a=[], b=[])
        for _ in range(a.rounds):
            sets["a"].append(timed(loop_a)[0])
            sets["b"].append(timed(loop_b)[0])
        da, db = stats(sets["a"]), stats(sets["b"])
        out["dataset_ms"] = dict(per_batch_host_loop=da, store_loop=db, scenes=a.scenes, batches=nb, sizes=sizes, detections=int(store.cursor[1]),
                                 fallbacks_in_timed_rounds=step.fallbacks - fb0, metrics_identical=identical)
        r, e = res["replay"], res["eager"]
        lines += [
            f"Step, B = {B} scenes x {a.points} points ({out['step_ms_per_batch']['rows']} live rows), bf16, voxel list {caps[0]} rows (ms per batch,",
            f"device events, medians of {a.rounds} alternating rounds after {a.warmup} warm-up rounds (min .. max)); replay valid: {valid0}:",
            f"  InferenceStep replay (packed dict):                     {fmt(r)}",
            f"  eager inf.simple_test_batched(..., on_device=True):     {fmt(e)}",
            ("  the replay is faster than the eager path beyond its measured spread." if r["max"] < e["min"] else
             "  the replay is NOT faster than the eager path beyond the measured spread."),
            f"Set of {a.scenes} scenes of {min(sizes)} .. {max(sizes)} points from files, BatchFeeder, B = {B} (ms per set, host clock, each loop ends in a",
            f"device synchronise; medians of {a.rounds} alternating rounds):",
            f"  (a) step.results() + IndoorEvaluator.add() per batch, compute(): {fmt(da)}   = {da['median'] / nb:.3f} ms per batch",
            f"  (b) test_dataset + DetStore, add_store(), compute():             {fmt(db)}   = {db['median'] / nb:.3f} ms per batch",
            f"  metric dicts identical: {identical}; eager fallbacks in the timed rounds: {out['dataset_ms']['fallbacks_in_timed_rounds']}",
            ("  (b) is faster than (a) beyond (a)'s measured spread." if db["median"] < da["min"] else
             "  (b) is NOT faster than (a) beyond (a)'s measured spread."),
        ]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--only", choices=("mean", "step"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "dynvox_bench measures the device path: it needs the GPU"
    assert a.scenes % a.batch == 0 and a.rounds >= 1 and a.calls >= 1
    dev = torch.device("cuda:0")
    cfg = copy.deepcopy(variants.scannet_large)
    out = dict(metric="dynvox_step_ab", points=a.points, batch=a.batch, features=FEAT, rounds=a.rounds, warmup=a.warmup)
    lines = [f"Dynamic voxelization in the captured inference step, ScanNet-large shape: B = {a.batch} x {a.points} points, {FEAT} features, "
             f"{cfg['pts_voxel_layer']['voxel_size'][0]} m voxels (MI355X)."]
    if a.only in (None, "mean"):
        mean_kernels(a, dev, cfg, lines, out)
    if a.only in (None, "step"):
        step_and_dataset(a, dev, cfg, lines, out)
    lines.append(json.dumps(out))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
