"""Dataset inference sharded over the GPUs of one node (GPU box; not part of bench.py): testing.ShardPlan + testing.test_dataset per rank,
det_store.gather_stores at the end (uni3detr_amd/det_store.py).

The set of tools/det_store_bench.py: 64 synthetic scenes of 20 000 points as .bin files, B = 8, bf16, a BatchFeeder into a captured
InferenceStep.  For every world size of 1, 2, 4, 8 the node has GPUs for, launch.spawn_ranks starts fresh processes, one per GPU, under
a time limit; every rank writes the files of its own share, captures its step from its own batches, and runs alternating rounds of
  (a) test_dataset over its share (at world 1: the unchanged one-device loop - the baseline), ending in a device synchronise;
  (b) the same followed by gather_stores, ending in a device synchronise - the whole set on every rank.
Rounds start behind a barrier; rank 0's host clock is reported.  gather_stores alone and u3d_det_store_merge alone (64 back-to-back
calls into one large store) are timed with device events on rank 0; at world 1 the merge is also timed at a dataset's size (6019
scenes over 8 synthetic shards).

    python tools/dist_test_bench.py [--scenes 64] [--batch 8] [--points 20000] [--rounds 10] [--warmup 2] [--worlds 1,2,4,8] [--out FILE]

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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

SEED = 77


def stats(xs):
    return dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3))


def merge_at_dataset_size(dev, n=6019, W=8, B=8, K=300, D=9, calls=8, rounds=20, warmup=3):
    """u3d_det_store_merge alone at the nuScenes-val size: n scenes of 0 .. K random rows (box_dim 9) dealt over W synthetic shards by
    ShardPlan, `calls` back-to-back merges into one store with room for all of them, device events -> (ms per call, rows per call)"""
    import torch

    from uni3detr_amd import native as nv
    from uni3detr_amd.det_store import DetStore
    from uni3detr_amd.testing import ShardPlan
    plan = ShardPlan(n, B, W)
    g = torch.Generator().manual_seed(0)
    counts = torch.randint(0, K + 1, (n,), generator=g, dtype=torch.int32)
    m = torch.from_numpy(plan.scene_map())
    per = [counts[m[:, 0] == r] for r in range(W)]                            # a shard's scenes in local order = in dataset order
    Smax, Nmax, total = max(len(c) for c in per), max(int(c.sum()) for c in per), int(counts.sum())
    sh_off = torch.zeros((W, Smax + 1), dtype=torch.int32)
    for r, c in enumerate(per):
        sh_off[r, 1:len(c) + 1] = torch.cumsum(c, 0)
    sh_head = torch.tensor([[len(c), int(c.sum())] for c in per], dtype=torch.int32)
    wire = [torch.rand((W, Nmax, D), generator=g), torch.rand((W, Nmax), generator=g),
            torch.randint(0, 10, (W, Nmax), generator=g, dtype=torch.int32), sh_off, sh_head]
    wire = [t.to(dev) for t in wire]
    big = DetStore(calls * n, K, D, dev, row_capacity=calls * total, invalid_capacity=0)
    scene_map = m.to(dev)
    ws = torch.empty((nv.det_store_merge_workspace(n),), dtype=torch.uint8, device=dev)
    ms = []
    for r in range(warmup + rounds):
        big.reset()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            nv.det_store_merge(*wire, scene_map, big.boxes, big.scores, big.labels, big.table, big.cursor, big.invalid, workspace=ws)
        e1.record()
        e1.synchronize()
        if r >= warmup:
            ms.append(e0.elapsed_time(e1) / calls)
    assert big.cursor.tolist() == [calls * n, calls * total, 0, 0] and torch.equal(big.table[:n, 1].cpu(), counts)
    return ms, total


def worker(a):
    import numpy as np
    import torch
    import torch.distributed as dist

    import projects.mmdet3d_plugin  # noqa: F401
    from oracle.weights import seeded_tensor
    from uni3detr_amd import datapath as dp
    from uni3detr_amd import evaluation as ev
    from uni3detr_amd import native as nv
    from uni3detr_amd import testing
    from uni3detr_amd.configs.sunrgbd import model as MODEL_CFG
    from uni3detr_amd.det_store import DetStore, exchange_stores, gather_stores
    from uni3detr_amd.feeder import BatchFeeder
    from uni3detr_amd.inference import InferenceModel, InferenceStep
    from uni3detr_amd.registry import build_model
    from uni3detr_amd.synth import room_scene

    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
    torch.cuda.set_device(dev)
    B = a.batch
    plan = testing.ShardPlan(a.scenes, B, world)
    mine, ids = plan.order(rank), plan.batch_ids(rank)
    assert ids, f"rank {rank} of {world} has no batch of {a.scenes} scenes in batches of {B}: nothing to capture a step from"
    pipeline = [dict(dp.SHIPPED_LOAD_ENTRIES["sunrgbd"]), dict(type="PointsRangeFilter", point_cloud_range=[-3.2, -0.2, -2.0, 3.2, 6.2, 0.56]),
                dict(type="DefaultFormatBundle3D"), dict(type="Collect3D")]
    tmp = tempfile.mkdtemp(prefix=f"dist_test_bench_{rank}_")
    try:
        samples, gts, labs = {}, [], []
        for k in range(a.scenes):
            p, g, l = room_scene(k, a.points)
            gts.append(torch.from_numpy(g).to(dev))
            labs.append(torch.from_numpy(l % 10).to(dev))
            if k in mine:                                                     # the colours are drawn per scene: every world size sees the same files
                path = os.path.join(tmp, f"scan{k}.bin")
                colour = np.random.default_rng(k).integers(0, 256, (a.points, 3)).astype(np.float32)
                np.concatenate([p[:, :3], colour], 1).tofile(path)
                samples[k] = dict(pts_filename=path)
        pipe = dp.DevicePipeline(pipeline, load=True)
        local = [samples[k] for k in mine]

        def sync_batch(j):                                                    # global batch j, which is one of this rank's
            recs = [dp.read_points(samples[k], pipe.load_cfg) for k in range(j * B, min((j + 1) * B, a.scenes))]
            return pipe(dp.pack_batch(None, raw=recs, device=dev))

        model = build_model(copy.deepcopy(MODEL_CFG))
        model.load_state_dict({k: seeded_tensor(k, tuple(v.shape), 3) for k, v in model.state_dict().items()})
        model = model.to(dev).set_precision("bf16").eval()
        num_classes = int(model.pts_bbox_head.num_classes)
        step = InferenceStep(InferenceModel(model), batch_size=B, point_capacity=a.points)
        step.capture(batches=[sync_batch(j) for j in ids], margin=1.25, warmup=3)
        K = int(step.det.boxes.shape[1])
        store = DetStore(len(mine), K, 7, dev)
        if world > 1:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)       # after the capture, as bench.py does

        def loop():
            store.reset()
            with BatchFeeder(local, range(len(local)), dp.DevicePipeline(pipeline, load=True), batch_size=B, device=dev,
                             drop_last=False) as f:
                testing.test_dataset(step, f, store, reload=sync_batch, on_batch=lambda j: torch.manual_seed(SEED + j), batch_ids=ids)

        def loop_and_gather():
            loop()
            return gather_stores(store, plan, num_classes=num_classes)

        def timed(fn):
            if world > 1:
                dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out

        for _ in range(a.warmup):
            loop()
            whole = loop_and_gather()
        fallbacks0 = step.fallbacks
        ms = dict(loop=[], gathered=[])
        for _ in range(a.rounds):                                             # alternating: both see the same machine
            ms["loop"].append(timed(loop)[0])
            ms["gathered"].append(timed(loop_and_gather)[0])

        # gather_stores alone (device events around the exchange and the merge; its two host reads are inside)
        gather_ms = []
        for r in range(a.warmup + a.rounds):
            if world > 1:
                dist.barrier()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            whole = gather_stores(store, plan, num_classes=num_classes)
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                gather_ms.append(e0.elapsed_time(e1))
        # u3d_det_store_merge alone: the exchanged shards, 64 back-to-back calls into a store with room for all of them
        wire, _ = exchange_stores(store, plan, num_classes=num_classes)
        rows = int(whole.cursor[1])
        big = DetStore(64 * a.scenes, K, 7, dev, row_capacity=max(64 * rows, 1), invalid_capacity=0)
        scene_map = torch.from_numpy(plan.scene_map()).to(dev)
        ws = torch.empty((nv.det_store_merge_workspace(a.scenes),), dtype=torch.uint8, device=dev)
        merge_ms = []
        for r in range(a.warmup + max(a.rounds, 20)):
            big.reset()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(64):
                nv.det_store_merge(*wire, scene_map, big.boxes, big.scores, big.labels, big.table, big.cursor, big.invalid, workspace=ws)
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                merge_ms.append(e0.elapsed_time(e1) / 64)
        assert big.cursor.tolist() == [64 * a.scenes, 64 * rows, 0, 0]
        e = ev.IndoorEvaluator(num_classes, device=dev)
        e.add_store(whole, gts, labs)
        metrics = e.compute()
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        if rank == 0:
            at_size = merge_at_dataset_size(dev) if world == 1 else None
            out = dict(merge_dataset_size_ms=at_size and dict(stats(at_size[0]), scenes=6019, shards=8, rows=at_size[1], box_dim=9),
                       world=world, loop_ms=stats(ms["loop"]), loop_and_gather_ms=stats(ms["gathered"]), gather_alone_ms=stats(gather_ms),
                       merge_alone_ms=stats(merge_ms), detections=rows, scenes_on_rank0=len(mine), max_num=K,
                       fallbacks_on_rank0=step.fallbacks - fallbacks0, mAP_025=metrics.get("mAP_0.25"))
            with open(a.result, "w") as fh:
                json.dump(out, fh)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=64)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--worlds", default="1,2,4,8")
    ap.add_argument("--rank-timeout", type=float, default=420.0, help="seconds one world size may take, all its ranks together")
    ap.add_argument("--out", default=None)
    ap.add_argument("--result", default=None, help=argparse.SUPPRESS)         # set for a rank: where rank 0 leaves its numbers
    a = ap.parse_args()
    if a.result:
        return worker(a)
    import torch

    from uni3detr_amd import launch
    gpus = torch.cuda.device_count()
    assert gpus >= 1, "dist_test_bench measures the device path: it needs the GPU"
    asked = [int(w) for w in a.worlds.split(",")]
    worlds = [w for w in asked if w <= min(gpus, 8) and a.scenes >= (w - 1) * a.batch + 1]
    tmp = tempfile.mkdtemp(prefix="dist_test_bench_")
    results = []
    try:
        for w in worlds:
            result = os.path.join(tmp, f"world{w}.json")
            argv = [sys.executable, os.path.abspath(__file__), "--scenes", str(a.scenes), "--batch", str(a.batch), "--points", str(a.points),
                    "--rounds", str(a.rounds), "--warmup", str(a.warmup), "--result", result]
            worst, codes = launch.spawn_ranks(w, argv, gpus, timeout_s=a.rank_timeout)
            assert worst == 0 and os.path.exists(result), f"world {w}: exit codes {codes}"
            with open(result) as fh:
                results.append(json.load(fh))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    base = results[0]["loop_ms"]
    lines = [f"Dataset inference over {a.scenes} scenes x {a.points} points, B = {a.batch}, bf16, BatchFeeder -> captured InferenceStep, sharded "
             f"by ShardPlan over the ranks (MI355X, {gpus} GPU(s) on the node).",
             f"Medians of {a.rounds} alternating rounds after {a.warmup} warm-up rounds (min .. max); every round starts behind a barrier and "
             "ends in a device synchronise; rank 0's clock."]
    for r in results:
        lines += [f"  world {r['world']}: test_dataset over the rank's share            {r['loop_ms']['median']:9.3f} ms  ({r['loop_ms']['min']:.3f} .. "
                  f"{r['loop_ms']['max']:.3f})" + ("   <- the one-device loop, unchanged: the baseline" if r["world"] == 1 else ""),
                  f"           ... followed by gather_stores (whole set on every rank) {r['loop_and_gather_ms']['median']:9.3f} ms  "
                  f"({r['loop_and_gather_ms']['min']:.3f} .. {r['loop_and_gather_ms']['max']:.3f})",
                  f"           gather_stores alone (device events)                    {r['gather_alone_ms']['median']:9.3f} ms  "
                  f"({r['gather_alone_ms']['min']:.3f} .. {r['gather_alone_ms']['max']:.3f})",
                  f"           u3d_det_store_merge alone (device events, {a.scenes} scenes, {r['detections']} rows, mean of 64 back-to-back calls) "
                  f"{r['merge_alone_ms']['median']:.4f} ms  ({r['merge_alone_ms']['min']:.4f} .. {r['merge_alone_ms']['max']:.4f})",
                  f"           mAP@0.25 {r['mAP_025']}, eager fallbacks on rank 0 in all rounds: {r['fallbacks_on_rank0']}"]
        d = r.get("merge_dataset_size_ms")
        if d:
            lines.append(f"           u3d_det_store_merge alone at a dataset's size (synthetic: {d['scenes']} scenes over {d['shards']} shards, {d['rows']} rows, "
                         f"box_dim {d['box_dim']}, mean of 8 back-to-back calls) {d['median']:.4f} ms  ({d['min']:.4f} .. {d['max']:.4f})")
    skipped = [w for w in asked if w not in worlds]
    if skipped:
        lines.append(f"  NOT measured: world {', '.join(map(str, skipped))} - the node exposes {gpus} GPU(s)"
                     + ("; scaling over ranks is unmeasured." if len(worlds) == 1 else "."))
    for r in results[1:]:
        g = r["loop_and_gather_ms"]
        lines.append(f"  world {r['world']} against the baseline: {g['median']:.3f} ms against {base['median']:.3f} ms = x{base['median'] / g['median']:.2f}"
                     + ("" if g["max"] < base["min"] else "  (NOT outside the baseline's measured spread)"))
    lines.append(json.dumps(dict(metric="dist_test_ab", scenes=a.scenes, batch=a.batch, points=a.points, rounds=a.rounds, warmup=a.warmup,
                                 gpus=gpus, worlds=results, not_measured=skipped)))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
