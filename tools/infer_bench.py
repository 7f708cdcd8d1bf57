"""Eval forward, ms per batch: InferenceModel (eval-mode BatchNorm folded into the convolutions), InferenceModel(sparse_levels=True)
(the sparse encoder's blocks and narrow strided convs folded too), InferenceModel(dense_fp8=True) (the wide dense convolutions on e4m3
operands, calibrated on the workload's own scenes), InferenceStep (the folded forward and the batched tail replayed as one hipGraph,
on top of the bf16 and of the fp8 InferenceModel) and model.eval(), same process, the paths alternating, medians (and min .. max) of
the samples after warm-up.  Needs the GPU.

    python tools/infer_bench.py [--reps 20] [--warmup 5]

Workloads: the benched SUN RGB-D shape (B = 8 scenes of 20 000 points) and a smaller batch (B = 2, 12 000 points), both on the
SUN RGB-D model in bf16 precision.  Per workload one JSON line: feature extractor (voxelize + encoder + SECOND3D + FPN) and the whole
simple_test_batched(on_device=True), unfolded, folded and folded with the sparse levels, detect_captured / detect_captured_fp8
(InferenceStep.run() on the same list of scenes, then the one event wait every path ends in; capacities measured on the workload's
own scenes, margin 1.25), whether every replay was valid, and the number of u3d_bn_apply launches per forward.
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import projects.mmdet3d_plugin  # noqa: E402,F401
from oracle.weights import seeded_tensor  # noqa: E402
from uni3detr_amd import native as nv  # noqa: E402
from uni3detr_amd.configs.sunrgbd import model as MODEL_CFG  # noqa: E402
from uni3detr_amd.inference import InferenceModel, InferenceStep  # noqa: E402
from uni3detr_amd.registry import build_model  # noqa: E402
from uni3detr_amd.synth import room_scene  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model = build_model(copy.deepcopy(MODEL_CFG))
    model.load_state_dict({k: seeded_tensor(k, tuple(v.shape), 3) for k, v in model.state_dict().items()})
    model = model.to(dev).set_precision("bf16").eval()
    inf = InferenceModel(model)
    inf_sp = InferenceModel(model, sparse_levels=True)
    inf_f8 = InferenceModel(model, dense_fp8=True)
    for name, B, npts in (("sunrgbd_b8_20000", 8, 20000), ("sunrgbd_b2_12000", 2, 12000)):
        pts = [torch.from_numpy(room_scene(i, npts)[0]).to(dev) for i in range(B)]
        inf_f8.calibrate([pts])
        step, step_f8 = (InferenceStep(i, batch_size=B, point_capacity=npts) for i in (inf, inf_f8))
        level_caps = [s_.capture(batches=[pts])[1] for s_ in (step, step_f8)][0]
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):      # (the unfolded head needs the autocast; the folded scope brings its own)
            paths = {
                "features_unfolded": lambda: model.extract_pts_feat(pts),
                "features_folded": lambda: inf.extract_pts_feat(pts),
                "features_folded_sparse": lambda: inf_sp.extract_pts_feat(pts),
                "features_folded_fp8": lambda: inf_f8.extract_pts_feat(pts),
                "detect_unfolded": lambda: model.simple_test_batched(None, pts, on_device=True),
                "detect_folded": lambda: inf.simple_test_batched(None, pts, on_device=True),
                "detect_folded_sparse": lambda: inf_sp.simple_test_batched(None, pts, on_device=True),
                "detect_folded_fp8": lambda: inf_f8.simple_test_batched(None, pts, on_device=True),
                "detect_captured": lambda: step.run(pts),
                "detect_captured_fp8": lambda: step_f8.run(pts),
            }
            calls = {}
            orig = nv.bn_apply
            for k in ("features_unfolded", "features_folded", "features_folded_sparse"):
                n = [0]

                def counting(*args, _n=n, **kw):
                    _n[0] += 1
                    return orig(*args, **kw)
                nv.bn_apply = counting
                try:
                    paths[k]()
                finally:
                    nv.bn_apply = orig
                calls[k] = n[0]
            # alternate the paths round by round: drift of the box hits both alike
            for fn in paths.values():
                timed(fn, 0, a.warmup)
            samples = {k: [] for k in paths}
            valid = True
            for _ in range(a.reps):
                for k, fn in paths.items():
                    samples[k] += timed(fn, 1, 0)
                valid = valid and int(step.valid) == 1 and int(step_f8.valid) == 1      # (read between the rounds, outside the timed spans)
        res = {k: round(statistics.median(v), 3) for k, v in samples.items()}
        res.update({k + "_min_max": [round(min(v), 3), round(max(v), 3)] for k, v in samples.items()})
        res.update(workload=name, batch=B, points=npts, reps=a.reps, bn_apply_unfolded=calls["features_unfolded"],
                   bn_apply_folded=calls["features_folded"], bn_apply_folded_sparse=calls["features_folded_sparse"],
                   folded_layers=len(inf.folded), unfolded_layers=len(inf.unfolded), folded_layers_sparse=len(inf_sp.folded),
                   unfolded_layers_sparse=len(inf_sp.unfolded), fp8_layers=len(inf_f8.fp8_layers), captured_valid=valid,
                   captured_level_capacities=level_caps)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
