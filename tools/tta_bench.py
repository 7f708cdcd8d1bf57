"""Stage times of double-flip test-time augmentation (A = 4 views) on KITTI- and nuScenes-shaped synthetic scenes (uni3detr_amd.synth)
with the shipped kitti_3classes / nuscenes models (seeded weights as built, eval mode).

    python tools/tta_bench.py [--scenes 2] [--iters 5] [--warmup 1]

Prints one JSON line: per config the median ms of (1) the view expansion plus the inner test pipeline, (2) the batched forward
(extract_pts_feat + head over B*A views), (3) get_bboxes over the views, (4) the device merge (merge_aug_batch: one kernel call for all
scenes and its one count read), (5) the NumPy restatement of the merge (tests/tta_ref.py) on the same candidates, and the candidate
counts behind them."""
import argparse
import ast
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import projects.mmdet3d_plugin  # noqa: E402,F401
import tta_ref as R  # noqa: E402
from uni3detr_amd import datapath as dp  # noqa: E402
from uni3detr_amd import tta  # noqa: E402
from uni3detr_amd.registry import build_model, to_config  # noqa: E402
from uni3detr_amd.synth import room_scene  # noqa: E402

SHIPPED = os.path.join(ROOT, "tests", "golden", "shipped_configs.txt")


def timed(fn, iters, warmup):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), out


def run(name, npts, B, iters, warmup, dev):
    cfg = to_config(ast.literal_eval(open(SHIPPED).read())[name]["config"]["model"])
    model = build_model(cfg).to(dev).eval()
    pc = tuple(cfg["pts_voxel_layer"]["point_cloud_range"])
    nfeat = cfg["pts_middle_encoder"]["in_channels"]
    raw = []
    for i in range(B):
        p = room_scene(i, npts, pc_range=pc)[0]
        if nfeat > 4:
            p = np.concatenate([p, np.zeros((p.shape[0], nfeat - 4), np.float32)], 1)
        raw.append(torch.from_numpy(p).to(dev))
    inner = [dict(type="GlobalRotScaleTrans", rot_range=[0, 0], scale_ratio_range=[1.0, 1.0], translation_std=[0, 0, 0]),
             dict(type="RandomFlip3D"), dict(type="PointsRangeFilter", point_cloud_range=list(pc))]
    pipe = dp.DevicePipeline([dict(type="MultiScaleFlipAug3D", img_scale=(1333, 800), pts_scale_ratio=1, flip=True, pcd_horizontal_flip=True,
                                   pcd_vertical_flip=True, transforms=inner)])
    packed = dp.pack_batch(raw, box_type_3d="LiDAR")
    t_exp, batch = timed(lambda: pipe(dict(packed, points=packed["points"].clone())), iters, warmup)
    points, metas = dp.tta_forward_inputs(batch)
    A = len(points)
    flat_p = [points[a][b] for b in range(B) for a in range(A)]
    flat_m = [metas[a][b] for b in range(B) for a in range(A)]
    head = model.pts_bbox_head

    def fwd():
        with torch.no_grad():
            feat, fps = model.extract_pts_feat(flat_p)
            return head(feat, flat_m, fps)
    t_fwd, outs = timed(fwd, iters, warmup)
    with torch.no_grad():
        t_bb, dets = timed(lambda: head.get_bboxes(outs, flat_m), iters, warmup)
    tab = tta.view_params(flat_m, dev)
    t_merge, merged = timed(lambda: tta.merge_aug_batch(dets, tab, A, tta.LIDAR, head.num_classes), iters, warmup)
    host = [[(d[0].cpu().numpy(), d[1].cpu().numpy(), d[2].cpu().numpy()) for d in dets[b * A:(b + 1) * A]] for b in range(B)]
    params = [(m["rot_degree"], m["pcd_scale_factor"], m["pcd_horizontal_flip"], m["pcd_vertical_flip"]) for m in flat_m[:A]]
    t0 = time.perf_counter()
    ref = [R.merge(h, params, R.LIDAR) for h in host]
    t_host = (time.perf_counter() - t0) * 1e3
    same = all(np.array_equal(r[2], m["labels_3d"].cpu().numpy()) for r, m in zip(ref, merged))
    return dict(scenes=B, views=A, points_per_scene=npts, candidates_per_scene=[sum(len(v[2]) for v in h) for h in host],
                merged_per_scene=[int(m["labels_3d"].numel()) for m in merged], labels_match_host=bool(same),
                expand_pipeline_ms=round(t_exp, 3), forward_ms=round(t_fwd, 3), get_bboxes_ms=round(t_bb, 3),
                merge_device_ms=round(t_merge, 3), merge_host_ms=round(t_host, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = dict(kitti=run("kitti_3classes", 20000, a.scenes, a.iters, a.warmup, dev),
               nuscenes=run("nuscenes", 60000, a.scenes, a.iters, a.warmup, dev))
    print(json.dumps(dict(tool="tta_bench", **res)))


if __name__ == "__main__":
    main()
