"""Uni3DETR detector behind the reference's registry name / constructor / method signatures (ref:
projects/mmdet3d_plugin/models/detectors/uni3detr.py:113-357; upstream MVXTwoStageDetector)."""
from collections import OrderedDict

import torch
import torch.distributed as dist
from torch import nn

from .. import native as nv
from ..shadow import ShadowSet
from ..registry import BACKBONES, DETECTORS, HEADS, MIDDLE_ENCODERS, NECKS, VOXEL_ENCODERS


class Voxelization(nn.Module):
    """mmcv.ops.Voxelization configuration holder (hard mode runs on u3d_voxelize_hard)."""

    def __init__(self, voxel_size, point_cloud_range, max_num_points, max_voxels=20000, deterministic=True):
        super().__init__()
        self.voxel_size, self.point_cloud_range = list(voxel_size), list(point_cloud_range)
        self.max_num_points = max_num_points
        self.max_voxels = tuple(max_voxels) if isinstance(max_voxels, (tuple, list)) else (max_voxels, max_voxels)
        self.deterministic = deterministic


@VOXEL_ENCODERS.register_module()
class HardSimpleVFE(nn.Module):
    def __init__(self, num_features=4):
        super().__init__()
        self.num_features = num_features
        self.fp16_enabled = False

    def forward(self, features, num_points, coors=None):
        return features[:, :, : self.num_features].sum(dim=1) / num_points.type_as(features).view(-1, 1)


@VOXEL_ENCODERS.register_module()
class DynamicSimpleVFE(nn.Module):
    """mean of the points of every occupied voxel; voxels come out in lexicographic (b,z,y,x) order like upstream's
    DynamicScatter -> torch.unique(dim=0).  Linear BitGrid rank + f32 atomics on the device (exact_mean: fixed-point
    integer sums instead, bits independent of the arrival order)."""

    def __init__(self, voxel_size=(0.2, 0.2, 4), point_cloud_range=(0, -40, -3, 70.4, 40, 1)):
        super().__init__()
        self.voxel_size, self.point_cloud_range = list(voxel_size), list(point_cloud_range)
        self.fp16_enabled = False
        # static-shape mode (hipGraph capture, set by TrainStep.measure_capacities): the voxel list has `capacity` rows, the real count
        # stays on the device (last_count_dev); None: exact size, one host read (as upstream's torch.unique)
        self.capacity = None
        self.last_count_dev = None
        # both off unless a caller turns them on for its own forward (InferenceStep._static, InferenceModel.scope):
        self.static_eval = False        # the capacity-sized route in eval mode too (a plain model.eval() forward stays exact-size)
        self.exact_mean = False         # order-free means (u3d_scatter_mean_exact) instead of f32 atomics: equal points, equal bits

    def grid_dims(self):
        vs, pr = self.voxel_size, self.point_cloud_range
        gx, gy, gz = (int(round((pr[3 + j] - pr[j]) / vs[j])) for j in range(3))
        return (gz, gy, gx)

    @torch.no_grad()
    def forward(self, features, coors, batch_size=None):
        """features f32 [N,F] (all scenes), coors int32 [N,4] (b,z,y,x) with -1 rows for dropped points."""
        coors = coors.int().contiguous()
        if batch_size is None:
            batch_size = int(coors[-1, 0].item()) + 1
        g = nv.BitGrid(batch_size, self.grid_dims(), features.device, linear=True)
        g.mark(coors)
        g.scan()
        self.last_count_dev = g.count_dev
        if self.capacity is None or not (self.training or self.static_eval):
            n_vox = int(g.count_dev.item())
        else:
            # no host read: capacity-sized list, ranks past it come back as -1 (their points are dropped; the step's capacity flag
            # reports it and the update is held - TrainStep - or the replay gated away - InferenceStep), rows past the count stay
            # (-1, ...) and zero
            n_vox = int(self.capacity)
            g.set_row_capacity(n_vox)
        rank = g.rank(coors)
        mean = nv.scatter_mean_exact if self.exact_mean else nv.scatter_mean
        feats, _ = mean(features.float().contiguous(), rank, n_vox)
        return feats, g.coords(n_vox)


FUSED_FPS_GLUE = True      # test-only module attribute: tests/test_toggles_gpu.py sets it False to run the tensor-op formulation of the
                           # glue around the FPS launch against the fused one (no environment switch reads it)


def shift_scale_points(pred_xyz, src_range, dst_range=None):
    """Affine map of [B,N,3] points from src_range=[min,max] to dst_range (default unit cube) (ref :18-46)."""
    lo, hi = src_range
    if dst_range is None:
        dlo, dhi = torch.zeros_like(lo), torch.ones_like(hi)
    else:
        dlo, dhi = dst_range
    return ((pred_xyz - lo[:, None, :]) * (dhi - dlo)[:, None, :]) / (hi - lo)[:, None, :] + dlo[:, None, :]


@DETECTORS.register_module()
class Uni3DETR(nn.Module):
    def __init__(self, dynamic_voxelization=False, use_grid_mask=False, pts_voxel_layer=None, pts_voxel_encoder=None,
                 pts_middle_encoder=None, pts_fusion_layer=None, pts_backbone=None, pts_neck=None, pts_bbox_head=None,
                 train_cfg=None, test_cfg=None, pretrained=None):
        super().__init__()
        self.pts_voxel_layer = Voxelization(**pts_voxel_layer) if pts_voxel_layer else None
        self.pts_voxel_encoder = VOXEL_ENCODERS.build(pts_voxel_encoder) if pts_voxel_encoder else None
        self.pts_middle_encoder = MIDDLE_ENCODERS.build(pts_middle_encoder) if pts_middle_encoder else None
        self.pts_backbone = BACKBONES.build(pts_backbone) if pts_backbone else None
        self.pts_neck = NECKS.build(pts_neck) if pts_neck else None
        if pts_bbox_head:
            head = dict(pts_bbox_head)
            head["train_cfg"] = train_cfg["pts"] if train_cfg else None
            head["test_cfg"] = test_cfg["pts"] if test_cfg and "pts" in test_cfg else None
            self.pts_bbox_head = HEADS.build(head)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.dynamic_voxelization = dynamic_voxelization
        if pts_middle_encoder:
            self.pts_fp16 = hasattr(self.pts_middle_encoder, "fp16_enabled")
        self.num_fps = pts_bbox_head["num_query"] if pts_bbox_head else 0
        # upstream furthest_point_sample is handed the raw [1,N,F] buffer and reads it as packed xyz triples
        # (DESIGN.md "FPS view"); set False to sample on true xyz instead.
        self.fps_packed_view = True
        self.amp_dtype = None           # torch.bfloat16 -> throughput mode (sparse encoder bf16 MFMA, dense + decoder autocast)
        self._fps_stream = None
        # FPS over sets above 20 480 points (several workgroups per set, native.fps): the caller's time-out record (int32 [2]; TrainStep
        # installs one and ORs [0] into the step's collective hold flag), the wait limit and the resident-workgroup budget
        self.fps_err, self.fps_poll_ticks, self.fps_max_wg = None, 0, 0
        self._shadows = None            # bf16 shadow set of the conv / linear parameters (uni3detr_amd/shadow.py)
        self.static_shapes = False      # True: capacity-sized tensors + device-side counts, no host reads (hipGraph capturable)

    with_pts_backbone = property(lambda self: self.pts_backbone is not None)
    with_pts_neck = property(lambda self: self.pts_neck is not None)

    def init_weights(self):
        return          # as the reference (ref :140-141): constructor-default init is what training really starts from

    def set_precision(self, mode):
        """'fp32': parity mode (exact-f32 MFMA everywhere); 'bf16': throughput mode (BASELINE configs[1]); 'mixed': the REFERENCE's
        recipe - SparseEncoderHD and SECOND3D in fp32 (ref: sparse_encoder_hd.py:62-64 fp16_enabled=False, uni3detr.py:150-151; the
        backbone is not wrapped in auto_fp16), neck + head in 16-bit (second3d_fpn.py:45 auto_fp16, uni3detr_sunrgbd.py:241
        fp16 loss scaling).  The fp32 modules keep f32 activations, statistics and parameters; their wide convolutions (channels % 64
        == 0) run as split-bf16 products - hi / lo bf16 planes, three MFMAs per product, f32 accumulation, ~2^-16 relative per product
        (uni3detr_amd/sparse.py split_scope; U3D_SPLIT_BF16=0 puts them back on the exact f32 MFMA at 1/16 of the bf16 rate) - the
        27-offset 16 / 32 / 64-channel levels as three accumulating split products on the direct-operand kernels; only the 4 -> 16
        input conv stays on the exact f32 kernel.
        'parity': the f32-GRADE mode with a throughput - every module in f32 storage (activations, statistics, parameters, losses);
        ALL convolutions (encoder, SECOND3D and the FPN) as split-bf16 products, decoder + head on the exact-f32 instantiation of the
        fused kernels.  It is at least as wide as the reference's own recipe everywhere (the reference autocasts neck + head to fp16)
        and is the mode whose box / class logits stay within 1e-3 of the fp32 oracle (tests/test_bf16_parity_gpu.py)."""
        assert mode in ("fp32", "bf16", "mixed", "parity")
        self.precision = mode
        self.amp_dtype = None if mode in ("fp32", "parity") else torch.bfloat16
        if self.pts_middle_encoder is not None:
            self.pts_middle_encoder.compute_dtype = torch.bfloat16 if mode == "bf16" else torch.float32
        dec = getattr(getattr(getattr(self, "pts_bbox_head", None), "transformer", None), "decoder", None)
        if dec is not None:
            dec.split_f32_wgrad = mode == "parity"      # the f32 decoder's parameter gradients as split-bf16 products (fused_decoder.py)
        return self

    # ------------------------------------------------------------------------------------------
    def _concat_points(self, pts):
        """list of [N_b,F] tensors, or a pre-packed dict(cat [sumN,F] f32, scene_off int32 [B+1] device, lens [B] ints)."""
        if isinstance(pts, dict):
            return pts["cat"], pts["scene_off"], list(pts["lens"])
        B = len(pts)
        lens = [int(p.shape[0]) for p in pts]
        cat = torch.cat([p.float() for p in pts]).contiguous() if B > 1 else pts[0].float().contiguous()
        off = [0]
        for n in lens:
            off.append(off[-1] + n)
        return cat, torch.tensor(off, dtype=torch.int32, device=cat.device), lens

    @staticmethod
    def _pack_points(pts):
        """Pre-pack a batch once (static input buffers for hipGraph replay)."""
        lens = [int(p.shape[0]) for p in pts]
        cat = torch.cat([p.float() for p in pts]).contiguous()
        off = [0]
        for n in lens:
            off.append(off[-1] + n)
        return dict(cat=cat, scene_off=torch.tensor(off, dtype=torch.int32, device=cat.device), lens=lens)

    def voxelize_batch(self, pts):
        """-> (coors [V,4] int32 (b,z,y,x), mean feats [V,F], voxel_off [B+1] device, points_cat, scene_off, lens)."""
        cat, scene_off, lens = self._concat_points(pts)
        B = len(lens)
        vl = self.pts_voxel_layer
        max_voxels = vl.max_voxels[0] if self.training else vl.max_voxels[1]
        _, coors, num, mean, voxel_off = nv.voxelize_hard(cat, scene_off, B, max(lens), vl.voxel_size, vl.point_cloud_range,
                                                          vl.max_num_points, max_voxels, want_voxels=False, want_mean=True)
        if self.static_shapes:
            total = coors.shape[0]                 # capacity B*max_voxels; rows past voxel_off[B] are (-1,...) and inert
        else:
            total = int(voxel_off[-1].item())      # the one host read the reference also has (ref :153)
        return coors[:total], mean[:total, : self.pts_voxel_encoder.num_features], voxel_off, cat, scene_off, lens

    def fps_queries(self, cat, scene_off, lens, coors, voxel_off):
        """2 x D-FPS per scene in ONE launch: raw points and float-cast (z,y,x) voxel coords (ref :178-189)."""
        B = len(lens)
        m = self.num_fps
        F_ = cat.shape[1]
        dev = cat.device
        max_n = max(max(lens), int(self.pts_voxel_layer.max_voxels[0 if self.training else 1]) if not self.dynamic_voxelization else 0)
        if (FUSED_FPS_GLUE and self.fps_packed_view and cat.is_cuda and cat.dtype == torch.float32 and cat.is_contiguous()
                and coors.dtype == torch.int32 and coors.is_contiguous() and coors.shape[1] == 4
                and scene_off.dtype == torch.int32 and voxel_off.dtype == torch.int32):
            # set descriptors + float voxel coordinates | the FPS rounds | gather + unit-cube map + concat: three launches
            return nv.fps_queries(cat, coors, scene_off, voxel_off, B, max_n, m, err=self.fps_err, poll_ticks=self.fps_poll_ticks,
                                  max_wg=self.fps_max_wg)[0]
        vox = coors[:, 1:].float().contiguous()                                           # [V,3] (z,y,x)
        if self.fps_packed_view:
            raw, raw_off = cat.reshape(-1), scene_off[:-1].long() * F_
        else:
            raw, raw_off = cat[:, :3].contiguous().reshape(-1), scene_off[:-1].long() * 3
        base = torch.cat([raw, vox.reshape(-1)])
        set_off = torch.cat([raw_off, raw.numel() + voxel_off[:-1].long() * 3])
        set_n = torch.cat([scene_off[1:] - scene_off[:-1], voxel_off[1:] - voxel_off[:-1]]).int()
        idx = nv.fps(base, set_off.contiguous(), set_n.contiguous(), max_n, m, err=self.fps_err, poll_ticks=self.fps_poll_ticks,
                     max_wg=self.fps_max_wg).long()                                       # [2B, m]
        p_idx = idx[:B] + scene_off[:-1].long()[:, None]
        v_idx = idx[B:] + voxel_off[:-1].long()[:, None]
        a = cat[:, :3][p_idx]                                                             # [B,m,3] xyz
        b = vox[v_idx].flip(-1)                                                           # [B,m,3] (z,y,x) -> (x,y,z) voxel coords
        a = shift_scale_points(a, [a.min(dim=1)[0], a.max(dim=1)[0]])
        b = shift_scale_points(b, [b.min(dim=1)[0], b.max(dim=1)[0]])
        return torch.cat([a, b], 1)

    def voxelize_dynamic_batch(self, pts):
        """ref :155-167: per-point coors (-1 rows kept), DynamicSimpleVFE mean per voxel."""
        cat, scene_off, lens = self._concat_points(pts)
        B = len(lens)
        vl = self.pts_voxel_layer
        coors = nv.voxelize_dynamic(cat, scene_off, B, vl.voxel_size, vl.point_cloud_range)
        feats, fcoors = self.pts_voxel_encoder(cat, coors, batch_size=B)
        return coors, feats, fcoors, cat, scene_off, lens

    def shadow_scope(self, refresh=True):
        """Context for ONE training forward in bf16 mode: refreshes the bf16 parameter shadows with one multi-tensor copy and
        lets every conv / linear use them instead of casting its own weights.  refresh=False: a later stage of the SAME forward
        (TrainStep's staged graphs) - the shadows are current, only the scope is entered."""
        import contextlib
        dev = next(self.parameters()).device
        if self.amp_dtype is None or dev.type != "cuda" or not torch.is_grad_enabled():
            return contextlib.nullcontext()
        if self._shadows is None or self._shadows.dtype != self.amp_dtype or self._shadows.params[0].device != dev:
            ps, convs = [], {}
            for m in self.modules():
                if isinstance(m, nn.Linear):
                    ps += [m.weight] + ([m.bias] if m.bias is not None else [])
                elif isinstance(m, nn.MultiheadAttention):
                    ps += [m.in_proj_weight, m.in_proj_bias]
                elif isinstance(m, nn.Conv3d):
                    convs[m.weight] = "oidhw"
            if self.pts_middle_encoder is not None:
                for p in self.pts_middle_encoder.parameters():
                    if p.dim() == 5:
                        convs[p] = "dhwio"
            self._shadows = ShadowSet(list({id(p): p for p in ps}.values()), self.amp_dtype, convs, flat=getattr(self, "_flat_params", None))
        return self._shadows.active(refresh)

    # The feature extractor in three stages, so that a captured training step can run stage 2 (the 300 serial FPS rounds, ~1 ms on
    # 2B CUs) as its OWN graph on a second stream next to stage 3: inside ONE hipGraph every node runs on a single hardware queue on this
    # stack (a rocprofv3 timeline of the replayed step shows k_fps alone on the device for its whole duration although it was
    # captured on a forked stream), so fork/join inside a capture buys no overlap.  extract_pts_feat() composes them for eager use.
    def stage_voxelize(self, pts):
        """-> dict: table coordinates + mean features (+ what the FPS stage needs)."""
        if self.dynamic_voxelization:
            coors, feats, fcoors, cat, scene_off, lens = self.voxelize_dynamic_batch(pts)
            # the voxel-coordinate FPS runs over the PER-POINT coors incl. -1 rows (ref :166,:183)
            return dict(coors=coors, feats=feats, fcoors=fcoors, cat=cat, scene_off=scene_off, lens=lens, voxel_off=scene_off)
        coors, feats, voxel_off, cat, scene_off, lens = self.voxelize_batch(pts)
        return dict(coors=coors, feats=feats, fcoors=coors, cat=cat, scene_off=scene_off, lens=lens, voxel_off=voxel_off)

    def stage_fps(self, v):
        return self.fps_queries(v["cat"], v["scene_off"], v["lens"], v["coors"], v["voxel_off"])

    def stage_features(self, v):
        from .. import sparse as sp
        # 'mixed': the fp32 modules' wide convs as split-bf16 products (sparse.split_scope) - f32 rows in and out, bf16 matrix pipe
        on = getattr(self, "precision", None) in ("mixed", "parity")
        if on and getattr(self, "_split3", None) is None:
            from .. import native as nv
            self._split3 = nv.Split3Set()        # this model's weight planes + job table: one refresh launch per step (native.Split3Set)
        with sp.split_scope(on, getattr(self, "_split3", None)):
            return self._stage_features(v)

    def _stage_features(self, v):
        x = self.pts_middle_encoder(v["feats"], v["fcoors"], len(v["lens"]))
        self._encoder_out = self._encoder_cut = None
        if getattr(self, "cut_encoder_backward", False) and torch.is_grad_enabled() and x.requires_grad:
            # cut point of TrainStep's two-phase backward: everything above sees a detached leaf; phase B feeds its gradient into x
            self._encoder_out = x
            x = self._encoder_cut = x.detach().requires_grad_(True)
        amp = self.amp_dtype
        with torch.autocast("cuda", dtype=amp, enabled=amp is not None):
            if self.with_pts_backbone:
                x = self.pts_backbone(x)              # follows the dtype of its input rows: fp32 in 'mixed' mode (the encoder's dense())
                self._backbone_out = self._backbone_cut = None
                if getattr(self, "cut_backbone_backward", False) and torch.is_grad_enabled() and isinstance(x, (tuple, list)) \
                        and all(t.requires_grad for t in x):
                    # second cut point of TrainStep's phased backward (SECOND3D outputs): the neck + head backward ends at these leaves,
                    # their gradient bucket is on the wire while the backbone's backward runs
                    self._backbone_out = tuple(x)
                    x = self._backbone_cut = tuple(t.detach().requires_grad_(True) for t in x)
            if self.with_pts_neck:
                if getattr(self, "precision", None) == "mixed":
                    x = tuple(t.to(torch.bfloat16) for t in x) if isinstance(x, (tuple, list)) else x.to(torch.bfloat16)
                x = self.pts_neck(x)
        return x

    def extract_pts_feat(self, pts):
        v = self.stage_voxelize(pts)
        # the FPS rounds only need points + voxel coords: on a side stream underneath the encoder / dense stack (eager launches overlap)
        cur = torch.cuda.current_stream()
        if self._fps_stream is None:
            self._fps_stream = torch.cuda.Stream()
        side = self._fps_stream
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            fpsbpts = self.stage_fps(v)
        x = self.stage_features(v)
        cur.wait_stream(side)
        for t in (v["cat"], v["coors"], v["voxel_off"], v["scene_off"]):
            t.record_stream(side)
        return x, fpsbpts

    def forward_pts_train(self, pts_feats, gt_bboxes_3d, gt_labels_3d, img_metas, gt_bboxes_ignore=None, fpsbpts=None):
        amp = self.amp_dtype
        with torch.autocast("cuda", dtype=amp, enabled=amp is not None):
            outs = self.pts_bbox_head(pts_feats, img_metas, fpsbpts)
        return self.pts_bbox_head.loss(gt_bboxes_3d, gt_labels_3d, outs)

    def forward(self, return_loss=True, **kwargs):
        return self.forward_train(**kwargs) if return_loss else self.forward_test(**kwargs)

    def forward_train(self, points=None, img_metas=None, gt_bboxes_3d=None, gt_labels_3d=None, gt_labels=None, gt_bboxes=None,
                      gt_bboxes_ignore=None):
        with self.shadow_scope():
            pts_feat, fpsbpts = self.extract_pts_feat(points)
            return dict(self.forward_pts_train(pts_feat, gt_bboxes_3d, gt_labels_3d, img_metas, gt_bboxes_ignore, fpsbpts))

    def forward_test(self, img_metas, points=None, **kwargs):
        if not isinstance(img_metas, list):
            raise TypeError(f"img_metas must be a list, but got {type(img_metas)}")
        if len(img_metas) == 1 or not isinstance(img_metas[0], list):
            metas = img_metas[0] if isinstance(img_metas[0], list) else img_metas
            return self.simple_test(metas, points, **kwargs)
        return self.aug_test(points, img_metas, **kwargs)

    def simple_test_pts(self, pts_feat, img_metas, rescale=False, fpsbpts=None):
        outs = self.pts_bbox_head(pts_feat, img_metas, fpsbpts)
        bbox_list = self.pts_bbox_head.get_bboxes(outs, img_metas, rescale=rescale)
        return [dict(boxes_3d=b.cpu(), scores_3d=s.cpu(), labels_3d=l.cpu()) for b, s, l in bbox_list]

    @torch.no_grad()
    def simple_test(self, img_metas, points=None, rescale=False):
        pts_feat, fpsbpts = self.extract_pts_feat(points)
        return self.simple_test_pts(pts_feat, img_metas, rescale=rescale, fpsbpts=fpsbpts)

    @torch.no_grad()
    def simple_test_batched(self, img_metas, points=None, rescale=False, on_device=False):
        """simple_test with the batched inference tail (Uni3DETRHead.get_bboxes_batched): the same list of dicts, from ONE copy per
        tensor for the whole batch (padded boxes / scores / labels and the counts), split on the host.  on_device=True returns the
        native.DetBatch itself (device tensors, no copy, no host sync for post_processing None / 'nms')."""
        pts_feat, fpsbpts = self.extract_pts_feat(points)
        outs = self.pts_bbox_head(pts_feat, img_metas, fpsbpts)
        det = self.pts_bbox_head.get_bboxes_batched(outs, img_metas, rescale=rescale)
        if on_device:
            return det
        return [dict(boxes_3d=b, scores_3d=s, labels_3d=l) for b, s, l in det.cpu().to_list()]

    @torch.no_grad()
    def aug_test(self, points, img_metas, imgs=None, rescale=False, max_batch=None, nms_thr=0.1, max_num=500, batched_tail=False):
        """Test-time augmentation (the reference's uni3detr.py:318-360 is marked "not done"; merge semantics: uni3detr_amd/tta.py).
        points[a][b], img_metas[a][b]: view a of sample b (the reference's forward_test shape, datapath.tta_forward_inputs).  All B*A
        views go through ONE batched extract_pts_feat + head forward (or chunks of whole samples of at most max_batch views), get_bboxes
        runs as in simple_test, and one device merge serves every sample.  Returns B dicts in simple_test's format (boxes_3d, scores_3d,
        labels_3d on the host) - not the reference's [dict(pts_bbox=...)] - so the evaluators take them unchanged.
        batched_tail=True feeds the merge from get_bboxes_batched instead of the per-view get_bboxes loop: the same detections."""
        from ..tta import coord_of, merge_aug_batch, view_params
        A, B = len(points), len(points[0])
        assert len(img_metas) == A and all(len(p) == B and len(m) == B for p, m in zip(points, img_metas))
        flat_p = [points[a][b] for b in range(B) for a in range(A)]              # scene-major, view-minor
        flat_m = [img_metas[a][b] for b in range(B) for a in range(A)]
        per = B if not max_batch else max(1, int(max_batch) // A)                 # samples per forward
        dets = []
        for b0 in range(0, B, per):
            ps, ms = flat_p[b0 * A:(b0 + per) * A], flat_m[b0 * A:(b0 + per) * A]
            pts_feat, fpsbpts = self.extract_pts_feat(ps)
            outs = self.pts_bbox_head(pts_feat, ms, fpsbpts)
            if batched_tail:                      # every view of the chunk through one device call, one host read (the counts)
                dets.extend(self.pts_bbox_head.get_bboxes_batched(outs, ms, rescale=rescale).to_list())
            else:
                dets.extend(self.pts_bbox_head.get_bboxes(outs, ms, rescale=rescale))
        dev = flat_p[0].device
        merged = merge_aug_batch(dets, view_params(flat_m, dev), A, coord_of(flat_m[0].get("box_type_3d", "Depth")),
                                 self.pts_bbox_head.num_classes, nms_thr, max_num)
        return [{k: v.cpu() for k, v in r.items()} for r in merged]

    @torch.no_grad()
    def aug_test_batched(self, batch_or_points, img_metas=None, *, tta_params=None, views=None, box_type_3d=None, on_device=False,
                         nms_thr=0.1, max_num=500):
        """aug_test with the whole tail on the device: ONE batched extract_pts_feat + head forward over all B*A views,
        get_bboxes_batched, then native.tta_merge_padded on the padded DetBatch as it is - the per-view counts never come to the host.
        Input, one of
          * the expanded packed dict a DevicePipeline with MultiScaleFlipAug3D returns (tta_views, tta_params, box_type_3d are its own;
            splitting it into scenes reads its offsets once);
          * points[a][b] / img_metas[a][b], aug_test's arguments (the view table is tta.view_params of the metas unless tta_params is given);
          * a flat list of B*A scenes, scene-major and view-minor, with views=A and tta_params f32 [B*A, 9] (box_type_3d: 'Depth' /
            'LiDAR', default 'Depth').
        on_device=True returns the merged native.DetBatch ([B, max_num, D], rows past count[b] zero) with no host read of a result;
        otherwise B dicts in simple_test's format from one copy per tensor.  The same detections as aug_test(batched_tail=True)."""
        from ..tta import coord_of, view_params
        from .. import native as nv
        flat_m = None
        if isinstance(batch_or_points, dict):
            from ..datapath import unpack_batch
            batch = batch_or_points
            if "tta_views" not in batch or "tta_params" not in batch:
                raise ValueError("aug_test_batched: the batch carries no tta_views / tta_params - run MultiScaleFlipAug3D in its pipeline")
            A = int(batch["tta_views"]) if views is None else int(views)
            tta_params = batch["tta_params"] if tta_params is None else tta_params
            box_type_3d = batch.get("box_type_3d", "Depth") if box_type_3d is None else box_type_3d
            flat_p = list(unpack_batch({k: batch[k] for k in ("points", "scene_off", "count") if k in batch})[0])
        elif len(batch_or_points) and isinstance(batch_or_points[0], (list, tuple)):
            points = batch_or_points
            A, B = len(points), len(points[0])
            assert img_metas is not None and len(img_metas) == A and all(len(p) == B and len(m) == B for p, m in zip(points, img_metas))
            flat_p = [points[a][b] for b in range(B) for a in range(A)]           # scene-major, view-minor
            flat_m = [img_metas[a][b] for b in range(B) for a in range(A)]
            if box_type_3d is None:
                box_type_3d = flat_m[0].get("box_type_3d", "Depth")
        else:
            flat_p = list(batch_or_points)
            if views is None or tta_params is None:
                raise ValueError("aug_test_batched: a flat list of scenes needs views= and tta_params=")
            A = int(views)
        if A < 1 or not flat_p or len(flat_p) % A:
            raise ValueError(f"aug_test_batched: {len(flat_p)} scenes are not a whole number of samples of {A} views")
        if tta_params is None:
            tta_params = view_params(flat_m, flat_p[0].device)
        if tuple(tta_params.shape) != (len(flat_p), nv.AUG_NPARAM):
            raise ValueError(f"aug_test_batched: tta_params must be [{len(flat_p)}, {nv.AUG_NPARAM}], got {tuple(tta_params.shape)}")
        pts_feat, fpsbpts = self.extract_pts_feat(flat_p)
        outs = self.pts_bbox_head(pts_feat, flat_m, fpsbpts)
        view_det = self.pts_bbox_head.get_bboxes_batched(outs, flat_m)
        det = nv.tta_merge_padded(view_det, tta_params.float().contiguous(), A, coord_of(box_type_3d or "Depth"), self.pts_bbox_head.num_classes,
                                  nms_thr, max_num)
        if on_device:
            return det
        return [dict(boxes_3d=b, scores_3d=s, labels_3d=l) for b, s, l in det.cpu().to_list()]

    # ------------------------------------------------------------------------------------------
    def pack_points(self, pts):
        return self._pack_points(pts)

    def _parse_losses(self, losses):
        log_vars = OrderedDict((k, v.mean() if isinstance(v, torch.Tensor) else sum(x.mean() for x in v)) for k, v in losses.items())
        loss = sum(v for k, v in log_vars.items() if "loss" in k)
        log_vars["loss"] = loss
        if dist.is_available() and dist.is_initialized():
            vals = torch.stack([v.detach() for v in log_vars.values()])
            dist.all_reduce(vals.div_(dist.get_world_size()))        # one message instead of one per log var
            log_vars = OrderedDict(zip(log_vars.keys(), vals.unbind()))
        return loss, log_vars

    def train_step(self, data, optimizer=None):
        losses = self(**data)
        loss, log_vars = self._parse_losses(losses)
        return dict(loss=loss, log_vars=log_vars, num_samples=len(data["img_metas"]) if data.get("img_metas") else len(data["points"]))
