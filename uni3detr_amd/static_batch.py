"""What a step over capacity-sized static buffers decides, stated once for TrainStep (trainer.py) and InferenceStep (inference.py):
the layout of the point / GT buffers and how a batch is bound into them, how the sparse levels are sized from sample batches, the ONE
device flag that says a replay must not be used, and the scaffold of a hipGraph capture.  Error texts take the caller's prefix."""
import gc

import torch

from . import native as nv


class StaticBatch:
    """The static input buffers of a step built for B scenes of up to P points each, allocated once: a graph keeps these addresses.
    `pts`: `cat` f32 [B * P, F] of which scene_off[B] rows are live (the detector and its kernels take `lens` = [P] * B as upper
    bounds and read the real extents from scene_off on the device).  One spare row behind `cat`: an empty LAST scene makes the FPS
    gather read the row at scene_off[B] (its value cannot matter: all samples of an empty set are that one row, the unit-cube map of
    a single point is 0 / 0).  `gts` (with gt_capacity=G): B * G rows of `gt_dim` columns, int32 labels, gt_off[B + 1], gmax = G."""

    def __init__(self, batch_size, point_capacity, feat, device, gt_capacity=None, gt_dim=None):
        B, P, G = int(batch_size), int(point_capacity), gt_capacity
        self.batch_size, self.point_capacity = B, P
        self.pts = dict(cat=torch.zeros((B * P + 1, int(feat)), dtype=torch.float32, device=device)[:B * P],
                        scene_off=torch.zeros(B + 1, dtype=torch.int32, device=device), lens=[P] * B)
        self.gts = None if G is None else dict(gt=torch.zeros((B * G, int(gt_dim)), dtype=torch.float32, device=device),
                                               labels=torch.zeros(B * G, dtype=torch.int32, device=device),
                                               gt_off=torch.zeros(B + 1, dtype=torch.int32, device=device), gmax=G)
        # [0]: the bound batch had a scene cut to P or G (added to the step's validity flag); counters: bind_packed calls that cut (points, boxes)
        self.ingest_flag = torch.zeros(1, dtype=torch.float32, device=device)
        self.ingest_over = torch.zeros(2, dtype=torch.int32, device=device)

    def bind_packed(self, batch, prefix):
        """Load the batch dict a DevicePipeline returns (points, scene_off[, count]; with GT buffers also gt_bboxes_3d, gt_off[,
        gt_count], gt_labels_3d) INTO the static buffers with u3d_batch_ingest on the current stream - no device-to-host copy, no host
        synchronisation.  The host checks what it knows without a read (scene count, columns, dtypes, devices); what only the device
        knows is handled there: a scene above the point capacity or above `gmax` boxes is cut to it and `ingest_flag` raised."""
        refuse_sweeps(batch, prefix)
        cat, B, gts = self.pts["cat"], self.batch_size, self.gts or {}
        pts, off, cnt = batch["points"], batch["scene_off"], batch.get("count")
        g, lab, go, gcnt = (batch.get(k) if gts else None for k in ("gt_bboxes_3d", "gt_labels_3d", "gt_off", "gt_count"))

        def i32(t, n, what):
            if t is not None and (t.dtype != torch.int32 or t.numel() != n or not t.is_contiguous()):
                raise ValueError(f"{prefix} {what} must be a contiguous int32 tensor of {n} elements")

        if not all(t is None or (torch.is_tensor(t) and t.device == cat.device) for t in (pts, off, cnt, g, lab, go, gcnt)):
            raise ValueError(f"{prefix} every tensor of the batch must live on {cat.device}")
        if pts.dim() != 2 or pts.dtype != torch.float32 or not pts.is_contiguous() or pts.shape[1] != cat.shape[1]:
            raise ValueError(f"{prefix} points must be contiguous float32 [n, {cat.shape[1]}], got {pts.dtype} {tuple(pts.shape)}")
        if off.numel() != B + 1:
            raise ValueError(f"{prefix} {off.numel() - 1} scenes, the step was built for {B}")
        i32(off, B + 1, "scene_off"); i32(cnt, B, "count")
        if g is not None:
            if g.dim() != 2 or g.dtype != torch.float32 or not g.is_contiguous() or g.shape[1] not in (7, 9):
                raise ValueError(f"{prefix} gt_bboxes_3d must be contiguous float32 [g, 7 | 9], got {g.dtype} {tuple(g.shape)}")
            if lab is None or go is None:
                raise ValueError(f"{prefix} gt_bboxes_3d needs gt_labels_3d and gt_off")
            i32(lab, g.shape[0], "gt_labels_3d"); i32(go, B + 1, "gt_off"); i32(gcnt, B, "gt_count")
        self.ingest_flag.zero_()
        nv.batch_ingest(pts, off, cnt, self.point_capacity, cat, self.pts["scene_off"], self.ingest_flag, gt=g, gt_labels=lab, gt_off=go,
                        gt_count=gcnt, gt_cap=int(gts.get("gmax", 0)), gt_out=gts.get("gt"), labels_out=gts.get("labels"),
                        gt_off_out=gts.get("gt_off"), overflow=self.ingest_over)

    def bind_scenes(self, model, points, prefix):
        """Load a list of batch_size per-scene tensors [n <= P, F] into the point buffers: the sizes are known on the host, so nothing is
        cut - a scene that does not fit raises before anything is written."""
        cat, P = self.pts["cat"], self.point_capacity
        if len(points) != self.batch_size:
            raise ValueError(f"{prefix} {len(points)} scenes, the step was built for {self.batch_size}")
        if any(p.dim() != 2 or int(p.shape[1]) != cat.shape[1] for p in points):
            raise ValueError(f"{prefix} points must have {cat.shape[1]} columns")
        if any(p.device != cat.device for p in points):
            raise ValueError(f"{prefix} every scene must live on {cat.device}")
        largest = max(int(p.shape[0]) for p in points)
        if largest > P:
            raise ValueError(f"{prefix} a scene of {largest} points exceeds point_capacity {P}")
        packed = model.pack_points(points)
        cat[:packed["cat"].shape[0]].copy_(packed["cat"])
        self.pts["scene_off"].copy_(packed["scene_off"])
        self.ingest_flag.zero_()


def refuse_sweeps(batch, prefix):
    if "sweeps" in batch:
        raise ValueError(f"{prefix} the batch still carries batch['sweeps'] - run the pipeline's LoadPointsFromMultiSweeps first")


def level_capacity(count, margin):
    """Rows a capacity-sized level gets for `count` rows seen: x margin, rounded up to a multiple of 256."""
    return ((int(count * margin) + 255) // 256) * 256


def max_level_counts(per_batch):
    """[[count per level] per sample batch] -> the largest count per level."""
    return [max(c) for c in zip(*per_batch)]


def fps_can_time_out(model, largest_set):
    """Only FPS over sets above native.FPS_REG_MAX points runs on several workgroups that wait for each other (fps_max_wg = 1: the
    single-workgroup streaming kernel whatever the size).  largest_set: the upper bound of what one scene hands to the FPS."""
    return getattr(model, "fps_max_wg", 0) != 1 and int(largest_set) > nv.FPS_REG_MAX


def validity_flag(model, caps, fps_err, ingest_flag, out):
    """out[0] (f32) <- > 0 iff this forward must not be used, computed on the device: a level over its capacity (the counts the encoder
    just produced against `caps`), the several-workgroup FPS timed out (`fps_err`, its record, or None when it cannot: passed as a
    "count" with capacity 0), or the bound batch was cut (`ingest_flag` or None)."""
    cnts, cps = [], []
    if caps is not None:
        cnts, cps = list(model.pts_middle_encoder.last_level_counts[1:1 + len(caps)]), list(caps)
        vfe = getattr(model, "pts_voxel_encoder", None)
        if getattr(vfe, "capacity", None) is not None and vfe.last_count_dev is not None:      # dynamic voxelization: the voxel list too
            cnts, cps = [vfe.last_count_dev] + cnts, [int(vfe.capacity)] + cps
    if fps_err is not None:
        cnts, cps = cnts + [fps_err[:1]], cps + [0]
    if cnts:
        nv.capacity_flag(cnts, cps, out)
    else:
        out.zero_()
    if ingest_flag is not None:
        out.add_(ingest_flag)


def drop_decoder_outputs(model):
    """Drop the decoder's cached outputs of an eager iteration (the caller: its own references first) BEFORE capturing: releasing them
    from inside a capture (when the attributes are re-assigned) tears down autograd nodes mid-capture and crashes hipStreamEndCapture."""
    dec = getattr(getattr(model.pts_bbox_head, "transformer", None), "decoder", None)
    if dec is not None:
        dec._reg_outputs = dec._states_c = dec._cls_outputs = dec._iou_outputs = dec._coord_outputs = dec._refs_sig = None
    gc.collect()
    torch.cuda.synchronize()


def warm_up(fn, n):
    """n calls of fn on a fresh side stream, ordered after and before the current stream's work -> that stream, to capture on."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(n):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    return s


def capture_graph(fn, stream, pool=None):
    """fn captured on `stream` -> the CUDAGraph (pool: a graph_pool_handle to share, None: a pool of its own)."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, pool=pool, stream=stream, capture_error_mode="thread_local"):
        fn()
    return g
