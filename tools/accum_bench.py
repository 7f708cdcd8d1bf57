"""The accumulating flat AdamW step (u3d_adamw_step_accum) beside the plain one (u3d_adamw_step_hold), at the SUN RGB-D model's flat
parameter count.  Needs the GPU.

    python tools/accum_bench.py [--reps 30] [--warmup 5] [--calls 10] [--steps 24] [--batch 8] [--points 20000] [--no-steps]

Line 1 (kind = "update_call"): device-event ms per call, the four paths alternating round by round, median of `--reps` samples of
`--calls` back-to-back calls each: an accumulate-only call, an applying call with and without EMA, and u3d_adamw_step_hold; with
the bytes each call has to move (f32 streams of n elements, counted from the kernels' loads and stores) and that over the time as
a fraction of the 8.0 TB/s HBM peak.
Lines 2.. (kind = "captured_step"): ms per captured training step (host clock between device synchronisations, rotating batches)
at accum_steps 1 (the default path: u3d_adamw_step_hold), 2 and 4, EMA off, same process.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import projects.mmdet3d_plugin  # noqa: E402,F401
from uni3detr_amd import native as nv  # noqa: E402
from uni3detr_amd.configs.sunrgbd import model as MODEL_CFG  # noqa: E402
from uni3detr_amd.plugin.structures import Boxes3D  # noqa: E402
from uni3detr_amd.registry import build_model  # noqa: E402
from uni3detr_amd.synth import room_scene  # noqa: E402
from uni3detr_amd.trainer import TrainStep  # noqa: E402

HBM_PEAK = 8.0e12
# f32 streams of n elements per call.  step_hold: grad (norm) + param, grad, 2 moments read + param, 2 moments written.
# accumulate-only: acc, grad read + acc written.  apply: those 3 + param, acc, 2 moments read + param, acc, 2 moments written; EMA: + 2.
STREAMS = dict(step_hold=8, accumulate_only=3, apply_no_ema=11, apply_ema=13)


def flat_count(model):
    """Elements of TrainStep's flat buffers: every parameter padded to a multiple of 64."""
    return sum((p.numel() + 63) // 64 * 64 for p in model.parameters() if p.requires_grad)


def events_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def update_calls(n, a, dev):
    torch.manual_seed(0)
    g = torch.randn(n, device=dev) * 1e-3
    ws = torch.empty(int(nv.lib().u3d_adamw_workspace(n)), dtype=torch.uint8, device=dev)

    def bufs(k, d, ema):
        b = dict(p=torch.randn(n, device=dev), m=torch.zeros(n, device=dev), v=torch.zeros(n, device=dev), acc=torch.zeros(n, device=dev),
                 ema=torch.zeros(n, device=dev) if ema else None, st=torch.zeros(16, device=dev), ast=torch.zeros(8, device=dev))
        nv.adamw_set_hyper(b["st"], 1e-4, (0.9, 0.999), 1e-8, 0.01, 10.0)
        nv.adamw_set_accum(b["ast"], k, d)
        return b

    acc_only, with_ema, no_ema, plain = bufs(1 << 24, None, False), bufs(1, 0.999, True), bufs(1, None, False), bufs(1, None, False)

    def accum(b):
        return lambda: nv.adamw_step_accum(b["p"], g, b["acc"], b["m"], b["v"], b["st"], b["ast"], ema=b["ema"], workspace=ws)

    paths = dict(accumulate_only=accum(acc_only), apply_ema=accum(with_ema), apply_no_ema=accum(no_ema),
                 step_hold=lambda: nv.adamw_step_state(plain["p"], g, plain["m"], plain["v"], plain["st"], workspace=ws))
    for fn in paths.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in paths}
    for _ in range(a.reps):                               # alternate the paths round by round: drift of the box hits all alike
        for k, fn in paths.items():
            samples[k].append(events_ms(fn, a.calls))
    outcomes = dict(accumulate_only=float(acc_only["ast"][5]), apply_ema=float(with_ema["ast"][5]), apply_no_ema=float(no_ema["ast"][5]))
    assert outcomes == dict(accumulate_only=0.0, apply_ema=1.0, apply_no_ema=1.0), outcomes      # each path did what its name says
    res = dict(kind="update_call", n=n, reps=a.reps, calls_per_sample=a.calls)
    for k, v in samples.items():
        ms = statistics.median(v)
        nbytes = STREAMS[k] * 4 * n
        res[k] = dict(ms=round(ms, 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4), MB=round(nbytes / 1e6, 1),
                      hbm_fraction=round(nbytes / (ms * 1e-3) / HBM_PEAK, 3))
    print(json.dumps(res), flush=True)


def batch(dev, B, npts, index):
    pts, gts, labels = [], [], []
    for i in range(B):
        p, g, l = room_scene(index * B + i, npts)
        gb = torch.from_numpy(g).clone()
        gb[:, 2] -= gb[:, 5] / 2
        pts.append(torch.from_numpy(p).to(dev)); gts.append(Boxes3D(gb).to(dev)); labels.append(torch.from_numpy(l).to(dev))
    return pts, gts, labels


def captured_steps(a, dev):
    rot = [batch(dev, a.batch, a.points, j) for j in range(4)]
    for k in (1, 2, 4):
        torch.manual_seed(1234)
        model = build_model(copy.deepcopy(MODEL_CFG)).to(dev).train().set_precision("bf16")
        ts = TrainStep(model, *rot[0], graph=True, accum_steps=k)
        snap = ts.snapshot()
        ts.capture(batches=rot)
        ts.restore(snap)
        packed = [(model.pack_points(p), model.pts_bbox_head.pack_gts(g, l, dev), None) for p, g, l in rot]
        it = 0
        for _ in range(8):
            ts.set_batch(*packed[it % 4]); it += 1
            ts.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            ts.set_batch(*packed[it % 4]); it += 1
            loss = ts.step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / a.steps * 1e3
        print(json.dumps(dict(kind="captured_step", accum_steps=k, entry="u3d_adamw_step_accum" if ts.accum else "u3d_adamw_step_hold",
                              batch=a.batch, points=a.points, steps=a.steps, ms_per_step=round(ms, 3), applied_updates=ts.applied_updates(),
                              held_steps=ts.held_steps(), nonfinite_skips=ts.nonfinite_skips(), loss=round(float(loss), 4))), flush=True)
        del ts, model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="back-to-back calls per timed sample")
    ap.add_argument("--steps", type=int, default=24, help="timed captured steps per accum_steps value (a multiple of 4: whole windows)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--no-steps", action="store_true", help="the update calls only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("accum_bench needs the GPU: a timing taken without one says nothing")
    dev = torch.device("cuda:0")
    update_calls(flat_count(build_model(copy.deepcopy(MODEL_CFG))), a, dev)
    if not a.no_steps:
        captured_steps(a, dev)


if __name__ == "__main__":
    main()
