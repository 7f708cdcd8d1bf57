"""python -m uni3detr_amd.train CONFIG [--work-dir DIR] ...: train a shipped point-cloud config end to end (the
counterpart of the reference's extra_tools/train.py).

The run: registry.Config.fromfile -> the model -> DevicePipeline(train_pipeline, load=True, + every opt-in the pipeline names) ->
datasets.samples_from_cfg -> a BatchFeeder per epoch -> point_capacity from the first batches (trainer.plan_point_capacity) ->
TrainStep(..., point_capacity=P, log=StepLog()) -> capture(batches=...) -> schedule.build_schedule -> training.fit.
A model with dynamic voxelization (ScanNet-large) trains on the fixed layout its pipeline's PointSample gives: point_capacity=None,
set_batch.  Validation (make_evaluate): InferenceModel + InferenceStep on the live weights, testing.test_dataset into a DetStore, the
evaluator of the dataset kind through add_store; the model is put back into training mode, its BatchNorm buffers are never written.
"""
import argparse
import os
import sys

import torch

CAPTURE_BATCHES = 4          # batches of the first epoch that size the point capacity and the sparse levels
OPT_IN = dict(LoadPointsFromMultiSweeps="sweeps", PointShuffle="point_shuffle", ObjectNameFilter="name_filter", ObjectNoise="object_noise",
              NormalizePointsColor="normalize_color")


def parse(argv=None):
    ap = argparse.ArgumentParser(prog="python -m uni3detr_amd.train", description=__doc__.split("\n\n")[0])
    ap.add_argument("config")
    ap.add_argument("--work-dir", default=None, help="checkpoints and log.json (default: work_dirs/<config name>)")
    ap.add_argument("--resume-from", default=None, help="a checkpoint of an earlier run: model, optimizer, EMA, log, epoch and iteration")
    ap.add_argument("--load-from", default=None, help="initial weights only")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-epochs", type=int, default=None, help="default: the config's runner.max_epochs / total_epochs")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "mixed", "parity", "fp32"])
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--no-validate", action="store_true")
    ap.add_argument("--log-interval", type=int, default=50)
    ap.add_argument("--accum-steps", type=int, default=1)
    ap.add_argument("--ema-decay", type=float, default=None)
    ap.add_argument("--trusted", action="store_true", help="allow the full (code-executing) unpickler for info files, database infos and "
                    "checkpoints that hold more than arrays")
    return ap.parse_args(argv)


def build_pipeline(pipeline_cfg, device, trusted=False, data_root=None):
    """DevicePipeline with the loader and every opt-in entry the pipeline names switched on; an ObjectSample entry gets its database
    from the entry's db_sampler (info_path: a plain pickle, so it needs `trusted`)."""
    from . import datapath as dp
    from .gtdb import GTDatabase
    types = [c["type"] for c in pipeline_cfg]
    kw = {flag: True for t, flag in OPT_IN.items() if t in types}
    db = None
    for c in pipeline_cfg:
        if c["type"] in ("ObjectSample", "UnifiedObjectSample") and c.get("db_sampler"):
            s = c["db_sampler"]
            if not trusted:
                raise RuntimeError(f"the pipeline's {c['type']} reads {s.get('info_path')}, a plain pickle: loading it runs the code it "
                                   "contains. If you trust the file pass --trusted")
            db = GTDatabase.from_infos(s["info_path"], s.get("data_root", data_root), s["classes"], s.get("prepare"),
                                       s.get("points_loader"), device=device)
    return dp.DevicePipeline(pipeline_cfg, gt_database=db, load=True, **kw)


def _scene_sizes(batch):
    return (batch["count"] if "count" in batch else batch["scene_off"][1:] - batch["scene_off"][:-1]).tolist()


def _sync_batch(samples, idx, pipe, box_type, device):
    """The batch of `idx` made synchronously (what a feeder yields, without its thread): for repairs and sample forwards."""
    from . import datapath as dp
    raw = [dp.read_points(samples[k], pipe.load_cfg) for k in idx]
    kw = {}
    if pipe.sweeps_cfg is not None:
        kw["sweeps"] = [dp.read_sweeps(samples[k]["info"], pipe.sweeps_cfg) for k in idx]
    return pipe(dp.pack_batch(None, None, box_type, raw=raw, device=device, **kw))


def make_evaluate(samples, meta, pipeline_cfg, batch_size, device, seed=0, capture_batches=2):
    """-> evaluate(ts, epoch) for training.fit over a validation split (datasets.samples_from_cfg of cfg.data.val).  The inference
    step is built and captured at the first call and kept; every call re-folds the current weights (InferenceModel.refresh - inside
    fit's ema_scope those are the EMA weights).  The head draws random query points in every eval forward: seeded per batch."""
    from . import datapath as dp
    from .det_store import DetStore
    from .feeder import BatchFeeder
    from .inference import InferenceModel, InferenceStep
    from .testing import test_dataset
    from .trainer import plan_point_capacity
    state = {}
    n, B, kind, box_type = len(samples), int(batch_size), meta["kind"], meta["box_type_3d"]
    if n < 1:
        raise ValueError("make_evaluate: the validation split is empty")

    types = {c["type"] for c in pipeline_cfg}

    def pipe():
        return dp.DevicePipeline(pipeline_cfg, load=True, sweeps="LoadPointsFromMultiSweeps" in types,
                                 normalize_color="NormalizePointsColor" in types)

    def batch_of(i, p):
        return _sync_batch(samples, list(range(i * B, min((i + 1) * B, n))), p, box_type, device)

    def evaluate(ts, epoch):
        model = ts.model
        if getattr(model, "precision", None) != "bf16":
            raise NotImplementedError("validation runs the folded bf16 inference path (InferenceModel): train with --precision bf16 or pass "
                                      "--no-validate")
        model.eval()
        try:
            with torch.no_grad():
                if "step" not in state:
                    p = pipe()
                    first = [batch_of(i, p) for i in range(min(int(capture_batches), n // B)) if (i + 1) * B <= n] or [batch_of(0, p)]
                    A = int(first[0].get("tta_views", 1))
                    P = plan_point_capacity([_scene_sizes(b) for b in first], margin=1.5)
                    inf = InferenceModel(model)
                    step = InferenceStep(inf, batch_size=B, point_capacity=P, views=A, box_type_3d=box_type)
                    step.capture(batches=[b if int(b["scene_off"].numel()) - 1 == B * A else dp.unpack_batch(b)[0] for b in first])
                    K = step.tta_max_num if A > 1 else int(step.det.boxes.shape[1])
                    state.update(step=step, inf=inf, K=K, dim=int(step.det.boxes.shape[2]), pipe=p)
                else:
                    state["inf"].refresh()
                step, p = state["step"], state["pipe"]
                store = DetStore(n, state["K"], state["dim"], device)
                on_batch = lambda i: torch.manual_seed(int(seed) * 7919 + i)       # noqa: E731
                with BatchFeeder(samples, range(n), pipe(), batch_size=B, device=device, box_type_3d=box_type, drop_last=False) as f:
                    test_dataset(step, f, store, reload=lambda i: batch_of(i, p), on_batch=on_batch)
                if kind == "indoor":
                    from .evaluation import IndoorEvaluator
                    ev = IndoorEvaluator(len(meta["classes"]), device=device)
                    ev.add_store(store, meta["gt_boxes"], meta["gt_labels"])
                    return ev.compute(label2cat=dict(enumerate(meta["classes"])))
                if kind == "kitti":
                    from .kitti_eval import KittiEvaluator
                    ev = KittiEvaluator(list(meta["classes"]), device=device)
                else:
                    from .nuscenes_eval import NuScenesEvaluator
                    ev = NuScenesEvaluator(list(meta["classes"]), device=device)
                ev.add_store(store, meta["infos"])
                return ev.compute()
        finally:
            model.train()
    return evaluate


def run(args, rank=0, world=1, local=0, printer=print):
    import projects.mmdet3d_plugin  # noqa: F401
    from . import datapath as dp
    from . import native as nv
    from .checkpoint import load_checkpoint
    from .datasets import samples_from_cfg
    from .feeder import BatchFeeder
    from .registry import Config, build_model
    from .schedule import build_schedule
    from .step_log import StepLog
    from .trainer import TrainStep, plan_point_capacity
    from .training import EpochPlan, fit, seed_epoch
    if not torch.cuda.is_available():
        raise SystemExit("train: needs a GPU (the hot path is HIP; there is no CPU fallback)")
    nv.lib()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    cfg = Config.fromfile(args.config)
    work_dir = args.work_dir or os.path.join("work_dirs", os.path.splitext(os.path.basename(args.config))[0])
    torch.manual_seed(args.seed)
    model = build_model(cfg["model"]).to(dev).train()
    model.set_precision(args.precision)
    if args.load_from:
        load_checkpoint(model, args.load_from, trusted=args.trusted)
    data = cfg["data"]
    B = int(data.get("samples_per_gpu", 1))
    samples, meta = samples_from_cfg(data["train"], trusted=args.trusted)
    pipeline_cfg = meta["pipeline"] or cfg["train_pipeline"]
    pipe = build_pipeline(pipeline_cfg, dev, trusted=args.trusted)
    plan = EpochPlan(len(samples), B, world=world, rank=rank, seed=args.seed, repeat=meta["repeat"], class_ids=meta["class_ids"])

    def make_feeder(order):
        return BatchFeeder(samples, order, pipe, batch_size=B, device=dev, box_type_3d=meta["box_type_3d"])

    # the first batches of epoch 0 size the point capacity and the sparse levels; fit() seeds the epoch again before it trains on them
    seed_epoch(args.seed, 0, rank)
    k = min(CAPTURE_BATCHES, plan.iters_per_epoch)
    with make_feeder(plan.order(0)[:k * B]) as f:
        first = list(f)
    opt, clip = cfg["optimizer"], ((cfg.get("optimizer_config") or {}).get("grad_clip") or {})
    common = dict(lr=float(opt["lr"]), weight_decay=float(opt.get("weight_decay", 0.01)), betas=tuple(opt.get("betas", (0.9, 0.999))),
                  max_norm=float(clip.get("max_norm", 0.0)), graph=True, accum_steps=args.accum_steps, ema_decay=args.ema_decay,
                  gt_capacity=max(64, 2 * max((len(s["gt_labels_3d"]) for s in samples), default=0)), log=StepLog(device=dev))
    if getattr(model, "dynamic_voxelization", False):
        lists = [dp.unpack_batch(b) for b in first]
        ts = TrainStep(model, *lists[0], point_capacity=None, **common)
    else:
        lists = first
        P = plan_point_capacity([_scene_sizes(b) for b in first])
        ts = TrainStep(model, *dp.unpack_batch(first[0]), point_capacity=P, **common)
    ts.capture(batches=lists)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29534")
        dist.init_process_group("nccl", device_id=dev)          # after the capture (TrainStep.enable_dist says why)
        ts.enable_dist()
    max_epochs = args.max_epochs or int((cfg.get("runner") or {}).get("max_epochs", cfg.get("total_epochs", 1)))
    evaluate, eval_interval = None, 0
    if not args.no_validate and data.get("val") is not None and rank == 0:
        val_samples, val_meta = samples_from_cfg(dict(data["val"], test_mode=True), trusted=args.trusted)
        evaluate = make_evaluate(val_samples, val_meta, val_meta["pipeline"] or cfg["test_pipeline"], B, dev, seed=args.seed)
        eval_interval = int((cfg.get("evaluation") or {}).get("interval", 1))
    ck_interval = int((cfg.get("checkpoint_config") or {}).get("interval", 1))
    return fit(ts, make_feeder, plan, build_schedule(cfg, plan.iters_per_epoch), max_epochs, log_interval=args.log_interval,
               work_dir=work_dir, checkpoint_interval=ck_interval, evaluate=evaluate, eval_interval=eval_interval, resume=args.resume_from,
               seed=args.seed, printer=printer)


def main(argv=None):
    args = parse(argv)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        from .launch import LaunchError, spawn_ranks
        try:
            worst, codes = spawn_ranks(args.gpus, [sys.executable, "-m", "uni3detr_amd.train"] + list(sys.argv[1:] if argv is None else argv),
                                       torch.cuda.device_count())
        except LaunchError as e:
            print(f"[train] {e}", file=sys.stderr, flush=True)
            raise SystemExit(2)
        if worst:
            print(f"[train] rank exit codes {codes}", file=sys.stderr, flush=True)
        raise SystemExit(worst)
    world, rank, local = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", "1"), ("RANK", "0"), ("LOCAL_RANK", "0")))
    if world != args.gpus:
        raise SystemExit(f"train: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    return run(args, rank, world, local)


if __name__ == "__main__":
    main()
