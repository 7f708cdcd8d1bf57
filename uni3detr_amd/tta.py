"""Test-time augmentation: the multi-view box merge (ref: projects/mmdet3d_plugin/core/merge_all_augs.py:9-98 with
core/bbox/util.py:82-102 bbox3d_mapping_back), on the device for all scenes of a batch at once (csrc/tta.hip, native.tta_merge).

Every view's boxes are mapped back with the inverse of the view (flip, rotate by -angle, scale by 1/scale: exactly a u3d_boxes_augment
call with those parameters), candidates are concatenated in view order (inside a view in get_bboxes order), non-finite scores are
dropped, every class (ascending, empty ones skipped) gets greedy rotated-BEV NMS at IoU > nms_thr (stable: equal scores go to the lower
concatenated index), and the kept boxes, class-major, are stably sorted by descending score and cut at max_num.  The results have
`simple_test`'s format (boxes_3d / scores_3d / labels_3d tensors), so the evaluators take them unchanged; the reference's aug_test
would have wrapped them as [dict(pts_bbox=...)], a path that never ran there.
"""
import numpy as np
import torch

from . import native as nv

DEPTH, LIDAR = 0, 1


def coord_of(box_type_3d):
    """'LiDAR' / 'Depth' (or a box class of that name) -> the kernels' coordinate code."""
    name = getattr(box_type_3d, "__name__", box_type_3d)
    return LIDAR if str(name).lower().startswith("lidar") else DEPTH


def view_params(metas, device):
    """metas of every view (flat list, scene-major, view-minor) -> f32 [V, 9] view table (flip_h, flip_v, sin, cos, angle, scale, 0, 0, 0)."""
    fh = np.array([bool(m.get("pcd_horizontal_flip", False)) for m in metas], np.float32)
    fv = np.array([bool(m.get("pcd_vertical_flip", False)) for m in metas], np.float32)
    ang = np.array([float(m.get("rot_degree", 0.0)) for m in metas], np.float32)
    sc = np.array([float(m.get("pcd_scale_factor", 1.0)) for m in metas], np.float32)
    tab = np.concatenate([np.stack([fh, fv, np.sin(ang), np.cos(ang), ang, sc], 1), np.zeros((len(metas), 3), np.float32)], 1)
    return torch.from_numpy(tab.astype(np.float32)).to(device)


def _tensor(b):
    return b.tensor if hasattr(b, "tensor") else b


def merge_aug_batch(dets, params, views, coord, num_classes, nms_thr=0.1, max_num=500):
    """dets: per view (B*views of them, scene-major, view-minor) (boxes [n, 7|9], scores [n], labels [n]) on one device; params: f32
    [B*views, 9] view table (view_params) -> B dicts(boxes_3d, scores_3d, labels_3d) on the device.  One kernel call for all scenes,
    one host sync (the per-scene counts)."""
    assert len(dets) % views == 0 and len(dets) == params.shape[0]
    dev = params.device
    boxes = [_tensor(d[0]).float() for d in dets]
    dim = next((b.shape[1] for b in boxes if b.dim() == 2 and b.shape[0]), boxes[0].shape[1] if boxes and boxes[0].dim() == 2 else 7)
    lens = [int(b.shape[0]) for b in boxes]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64).tolist()
    cat = (torch.cat([b.reshape(-1, dim) for b in boxes]).to(dev) if off[-1] else torch.zeros((0, dim), device=dev))
    scores = torch.cat([d[1].reshape(-1).float() for d in dets]).to(dev) if off[-1] else torch.zeros((0,), device=dev)
    labels = torch.cat([d[2].reshape(-1).to(torch.int32) for d in dets]).to(dev) if off[-1] else torch.zeros((0,), dtype=torch.int32, device=dev)
    ob, os_, ol, oc = nv.tta_merge(cat, scores, labels, off, params, views, coord, num_classes, nms_thr, max_num)
    cnt = oc.cpu().tolist()                                   # the one host sync
    return [dict(boxes_3d=ob[b, :c], scores_3d=os_[b, :c], labels_3d=ol[b, :c].long()) for b, c in enumerate(cnt)]


def merge_all_aug_bboxes_3d(aug_results, img_metas, test_cfg=None, nms_thr=0.1, max_num=500):
    """The reference's signature, one sample: aug_results per view dict(boxes_3d, scores_3d, labels_3d); img_metas per view [meta]
    (or meta).  The reference hard-codes nms_thr 0.1 and max_num 500 and ignores test_cfg; so does this.  The class count is the
    largest label + 1 (the reference's one .item() sync)."""
    assert len(aug_results) == len(img_metas), (len(aug_results), len(img_metas))
    metas = [m[0] if isinstance(m, (list, tuple)) else m for m in img_metas]
    dev = next((_tensor(r["boxes_3d"]).device for r in aug_results if _tensor(r["boxes_3d"]).is_cuda), torch.device("cuda"))
    dets = [(_tensor(r["boxes_3d"]).to(dev), r["scores_3d"].to(dev), r["labels_3d"].to(dev)) for r in aug_results]
    ncls = max([int(d[2].max()) + 1 for d in dets if d[2].numel()] + [1])
    return merge_aug_batch(dets, view_params(metas, dev), len(dets), coord_of(metas[0].get("box_type_3d", "Depth")), ncls, nms_thr,
                           max_num)[0]
