"""Time of the GT-paste database crop (csrc/gtdb.hip) on nuScenes-shaped and KITTI-shaped synthetic scenes (synth.gtdb_scenes) against
the NumPy restatement of the reference's loop (tests/gtdb_ref.py) and against the parent path GTDatabase.from_scenes (a point x box bit
matrix and a Python loop over the objects), on the same input.

    python tools/gtdb_bench.py [--scenes 8] [--iters 5]

Prints one JSON line; per data-set shape: device ms per scene for the count / scan / crop entry points (events around each, median of
--iters chunks of --scenes scenes), upload ms per scene (wall clock around the host-to-device copy of points and boxes, synchronised),
ms per scene of create_groundtruth_database as a whole (upload, crop, host read, info dicts), of the host restatement and of
from_scenes, the bytes the two passes have to move (scene points read twice for columns 0-2 resp. all columns, object rows written
once) and what that costs at --hbm-gbs.  Reported, not gated."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import gtdb_ref as R  # noqa: E402
from uni3detr_amd import gtdb as G  # noqa: E402
from uni3detr_amd import native as nv  # noqa: E402
from uni3detr_amd.synth import gtdb_scenes  # noqa: E402


def _med(v):
    return float(np.median(v))


def run(kind, n_scenes, iters, hbm_gbs):
    scenes = gtdb_scenes(kind, n_scenes, seed=1)
    classes = sorted({str(n) for s in scenes for n in s["gt_names"]})
    builder = G.DbInfoBuilder(kind)
    metas = [builder.select(s) for s in scenes]
    pts_h = np.concatenate([s["points"] for s in scenes])
    box_h = np.concatenate([m["boxes"][m["gt_idx"]] for m in metas])
    lens, gl = [len(s["points"]) for s in scenes], [len(m["gt_idx"]) for m in metas]
    up, dev_ms = [], {"gtdb_count": [], "gtdb_scan": [], "gtdb_crop": []}
    for it in range(iters + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P, B = torch.from_numpy(pts_h).cuda(), torch.from_numpy(box_h).cuda()
        so = torch.tensor(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)).cuda()
        bo = torch.tensor(np.concatenate([[0], np.cumsum(gl)]).astype(np.int32)).cuda()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        nv.TIMER = nv.KernelTimer()
        try:
            out, off, num = nv.gtdb_crop(P, so, None, max(lens), B, bo, max_boxes=max(gl))
            calls = nv.TIMER.durations_ms()
        finally:
            nv.TIMER = None
        if it:                                              # the first chunk warms up
            up.append((t1 - t0) * 1e3 / n_scenes)
            for tag, ms in calls:
                dev_ms[tag].append(ms / n_scenes)
    obj_rows, feat = int(out.shape[0]), int(out.shape[1])
    moved = pts_h.shape[0] * 12 + pts_h.shape[0] * feat * 4 + obj_rows * feat * 4
    whole = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        G.create_groundtruth_database(scenes, classes, info_prefix=kind, chunk_scenes=n_scenes)
        torch.cuda.synchronize()
        whole.append((time.perf_counter() - t0) * 1e3 / n_scenes)
    t0 = time.perf_counter()
    R.create_groundtruth_database(scenes[:2], kind)
    host = (time.perf_counter() - t0) * 1e3 / 2
    cat = {n: i for i, n in enumerate(classes)}
    dp_, db_, dl_ = ([torch.from_numpy(s["points"]).cuda() for s in scenes], [torch.from_numpy(m["boxes"][m["gt_idx"]]).cuda() for m in metas],
                     [torch.tensor([cat[str(m["names"][i])] for i in m["gt_idx"]], dtype=torch.int64).cuda() for m in metas])
    parent = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        G.GTDatabase.from_scenes(dp_, db_, dl_, classes)
        torch.cuda.synchronize()
        parent.append((time.perf_counter() - t0) * 1e3 / n_scenes)
    dev = {k.replace("gtdb_", "") + "_ms_per_scene": _med(v) for k, v in dev_ms.items()}
    passes = dev["count_ms_per_scene"] + dev["crop_ms_per_scene"]
    return dict(scenes=n_scenes, points_per_scene=int(np.mean(lens)), boxes_per_scene=float(np.mean(gl)), feat=feat, box_dim=int(box_h.shape[1]),
                object_rows_per_scene=obj_rows / n_scenes, **dev, upload_ms_per_scene=_med(up), build_ms_per_scene=min(whole),
                host_restatement_ms_per_scene=host, from_scenes_ms_per_scene=min(parent), bytes_moved_per_scene=moved / n_scenes,
                hbm_bound_ms_per_scene=moved / n_scenes / (hbm_gbs * 1e9) * 1e3,
                hbm_fraction=(moved / n_scenes / (hbm_gbs * 1e9) * 1e3) / passes if passes > 0 else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="peak HBM bandwidth the bound is priced at (MI355X: 8 TB/s)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    res = dict(device=torch.cuda.get_device_name(0), nuscenes=run("nuscenes", a.scenes, a.iters, a.hbm_gbs),
               kitti=run("kitti", a.scenes, a.iters, a.hbm_gbs))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
