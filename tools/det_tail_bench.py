"""The inference tail on synthetic head outputs: the per-scene path (Uni3DETRHead.get_bboxes + the three .cpu() copies per scene of
simple_test_pts) against the batched one (get_bboxes_batched + .to_list(): one device call, one count read), in ms per batch.

    python tools/det_tail_bench.py [--iters 30] [--warmup 5] [--timeout 120]

Shapes: nuscenes (B=4, Q=900, C=10, K=900, nms 0.2, num_thr 500, 9 box columns), sunrgbd (B=4, Q=300, C=10, K=1000, nms 0.5), scannet
(B=3, Q=300, C=18, K=5000, no post-processing), tta16 (the nuscenes shape with the 16 views of a double-flip batch of 4 samples),
nuscenes_b1 (one scene), kitti_b1 / kitti_b8 / kitti_b16 (Q=300, C=3, K=150, box_merging with the shipped per-class score_thr) and
sunrgbd_soft (the sunrgbd shape with soft_nms).  Every case runs in a process of its own under `timeout`; the first failure ends the run.  One JSON line per
case: per_scene_ms, batched_ms (device slices from .to_list()) and batched_host_ms (.cpu().to_list(): host tensors, the end state of
the per-scene number), medians of wall time with a device synchronisation after every repetition - each with its [min, max] under
*_range_ms -, and whether the two paths agree."""
import argparse
import copy
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = dict(
    nuscenes=dict(B=4, Q=900, C=10, K=900, dim=9, spread=12.0, pp=dict(type="nms", nms_thr=0.2, num_thr=500)),
    sunrgbd=dict(B=4, Q=300, C=10, K=1000, dim=7, spread=2.0, pp=dict(type="nms", nms_thr=0.5)),
    scannet=dict(B=3, Q=300, C=18, K=5000, dim=7, spread=2.0, pp=None),
    tta16=dict(B=16, Q=900, C=10, K=900, dim=9, spread=12.0, pp=dict(type="nms", nms_thr=0.2, num_thr=500)),
    nuscenes_b1=dict(B=1, Q=900, C=10, K=900, dim=9, spread=12.0, pp=dict(type="nms", nms_thr=0.2, num_thr=500)),
    kitti_b1=dict(B=1, Q=300, C=3, K=150, dim=7, spread=12.0, pp=dict(type="box_merging", score_thr=[0.0, 0.3, 0.65])),
    kitti_b8=dict(B=8, Q=300, C=3, K=150, dim=7, spread=12.0, pp=dict(type="box_merging", score_thr=[0.0, 0.3, 0.65])),
    kitti_b16=dict(B=16, Q=300, C=3, K=150, dim=7, spread=12.0, pp=dict(type="box_merging", score_thr=[0.0, 0.3, 0.65])),
    sunrgbd_soft=dict(B=4, Q=300, C=10, K=1000, dim=7, spread=2.0, pp=dict(type="soft_nms", gaussian_sigma=0.3, prune_threshold=1e-3)),
)


def run_case(name, iters, warmup):
    import numpy as np
    import torch

    import projects.mmdet3d_plugin  # noqa: F401
    from uni3detr_amd.configs.sunrgbd import model as MODEL_CFG
    from uni3detr_amd.plugin.bbox import NMSFreeCoder
    from uni3detr_amd.registry import build_model
    c = CASES[name]
    dev = torch.device("cuda:0")
    head = build_model(copy.deepcopy(MODEL_CFG)).pts_bbox_head.eval()          # only bbox_coder / post_processing / num_classes are read
    head.num_classes, head.post_processing = c["C"], c["pp"]
    rng = [-100.0] * 3 + [100.0] * 3
    head.bbox_coder = NMSFreeCoder(pc_range=rng, post_center_range=rng, max_num=c["K"], alpha=0.5, num_classes=c["C"])
    g = torch.Generator().manual_seed(0)
    L, B, Q = 3, c["B"], c["Q"]
    r = lambda *s: torch.randn(*s, generator=g)
    code = [r(L, B, Q, 2) * c["spread"], r(L, B, Q, 2) * 0.3 + 0.5, r(L, B, Q, 1), r(L, B, Q, 1) * 0.3, r(L, B, Q, 2)]
    if c["dim"] == 9:
        code.append(r(L, B, Q, 2))
    preds = dict(all_cls_scores=(r(L, B, Q, c["C"]) - 2.0).to(dev), all_bbox_preds=torch.cat(code, -1).to(dev),
                 all_iou_preds=r(L, B, Q, 1).to(dev))

    def per_scene():
        return [(b.cpu(), s.cpu(), l.cpu()) for b, s, l in head.get_bboxes(preds, None)]

    def timed(fn):
        for _ in range(warmup):
            out = fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return (float(np.median(ts)), float(np.min(ts)), float(np.max(ts))), out

    with torch.no_grad():
        t_ref, ref = timed(per_scene)
        t_dev, _ = timed(lambda: head.get_bboxes_batched(preds, None).to_list())
        t_host, got = timed(lambda: head.get_bboxes_batched(preds, None).cpu().to_list())
    same = all(all(torch.equal(x, y) for x, y in zip(a, b)) for a, b in zip(got, ref))
    print(json.dumps(dict(tool="det_tail_bench", case=name, B=B, Q=Q, C=c["C"], K=c["K"], post_processing=c["pp"],
                          kept_per_scene=[int(x[1].numel()) for x in ref], per_scene_ms=round(t_ref[0], 3), batched_ms=round(t_dev[0], 3),
                          batched_host_ms=round(t_host[0], 3), per_scene_range_ms=[round(v, 3) for v in t_ref[1:]],
                          batched_range_ms=[round(v, 3) for v in t_dev[1:]], batched_host_range_ms=[round(v, 3) for v in t_host[1:]],
                          identical=bool(same))), flush=True)
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per case")
    ap.add_argument("--case", choices=sorted(CASES), help="run this one case in this process")
    a = ap.parse_args()
    if a.case:
        return run_case(a.case, a.iters, a.warmup)
    for name in CASES:
        rc = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--case", name, "--iters",
                             str(a.iters), "--warmup", str(a.warmup)]).returncode
        if rc != 0:
            print(json.dumps(dict(tool="det_tail_bench", case=name, failed=rc)), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
