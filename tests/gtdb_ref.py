"""NumPy restatement of the object-database loop of the reference's extra_tools/data_converter/create_unified_gt_database.py (lines
85-176, the image part left out), for the tests of uni3detr_amd.gtdb.  RESTATED, PARITY UNPINNED: the loop calls mmdet3d's
box_np_ops.points_in_rbbox, which is not part of the reference tree, so the inside test is the strict six-face predicate restated in
tests/objaug_ref.py (float64) and nothing here was run against the original.  Written from the script's behaviour, scene by scene:

    point_indices = points_in_rbbox(points, boxes)            [n, g] bool
    for i in range(g):
        gt_points = points[point_indices[:, i]]; gt_points[:, :3] -= boxes[i, :3]      (float32, scene order kept)
        if used_classes is None or names[i] in used_classes:  one info dict, the group-id counter advances

The data set side (NuScenesSweepDataset with use_valid_flag=True) drops boxes whose valid flag is false before the loop sees them.
"""
import os

import numpy as np

from objaug_ref import points_in_rbbox


def crop_scene(points, boxes):
    """-> list of g float32 arrays [n_i, F]: the script's gt_points of every box."""
    points = np.asarray(points, np.float32)
    boxes = np.asarray(boxes, np.float32).reshape(-1, np.shape(boxes)[-1] if np.ndim(boxes) == 2 else 7)
    inside = np.zeros((len(points), len(boxes)), bool)
    for s in range(0, len(points) if len(boxes) else 0, 65536):      # chunks keep the [n, g] float64 temporaries small
        inside[s:s + 65536] = points_in_rbbox(points[s:s + 65536], boxes[:, :7])
    out = []
    for i in range(len(boxes)):
        g = points[inside[:, i]].copy()
        g[:, :3] -= boxes[i, :3]
        out.append(g)
    return out


def create_groundtruth_database(scenes, info_prefix, used_classes=None):
    """scenes: dicts as uni3detr_amd.gtdb.create_groundtruth_database takes them (host arrays, sweeps already merged).
    -> (all_db_infos, objects): objects[k] = list of the float32 point arrays of db_infos[k], same order."""
    all_db_infos, objects = {}, {}
    group_counter = 0
    for sc in scenes:
        boxes = np.asarray(sc["gt_bboxes_3d"], np.float32)
        boxes = boxes.reshape(-1, boxes.shape[-1] if boxes.ndim == 2 else 7)
        names = np.asarray(sc["gt_names"]).reshape(-1)
        mask = np.ones(len(boxes), bool) if sc.get("valid_flag") is None else np.asarray(sc["valid_flag"], bool)
        boxes, names = boxes[mask], names[mask]
        group_ids = np.arange(len(boxes), dtype=np.int64) if sc.get("group_ids") is None else np.asarray(sc["group_ids"])[mask]
        difficulty = np.zeros(len(boxes), np.int32) if sc.get("difficulty") is None else np.asarray(sc["difficulty"])[mask]
        score = None if sc.get("score") is None else np.asarray(sc["score"])[mask]
        crops = crop_scene(sc["points"], boxes)
        group_dict = {}
        for i in range(len(boxes)):
            if used_classes is not None and names[i] not in used_classes:
                continue
            name = str(names[i])
            info = {"name": name,
                    "path": os.path.join(f"{info_prefix}_gt_database", "pts_dir", f"{sc['sample_idx']}_{name}_{i}.bin"),
                    "image_idx": sc["sample_idx"], "image_path": "", "image_crop_key": "", "image_crop_depth": 0, "gt_idx": i,
                    "box3d_lidar": boxes[i], "num_points_in_gt": crops[i].shape[0], "difficulty": difficulty[i]}
            local = group_ids[i].item()
            if local not in group_dict:
                group_dict[local] = group_counter
                group_counter += 1
            info["group_id"] = group_dict[local]
            if score is not None:
                info["score"] = score[i]
            all_db_infos.setdefault(name, []).append(info)
            objects.setdefault(name, []).append(crops[i])
    return all_db_infos, objects


def key_major(all_db_infos, objects, feat):
    """-> (points [P, feat] f32, obj_off int64 [D+1]): the objects key after key, as GTDatabase.from_infos lays them out."""
    flat = [o for k in all_db_infos for o in objects[k]]
    off = np.concatenate([[0], np.cumsum([len(o) for o in flat])]).astype(np.int64)
    pts = np.concatenate(flat).astype(np.float32) if flat else np.zeros((0, feat), np.float32)
    return pts.reshape(-1, feat), off


def face_distance(points, boxes):
    """[n, g] float64: the distance of every point to the nearest of the six face planes of every box."""
    b = np.asarray(boxes, np.float64)
    out = np.zeros((len(points), len(b)))
    for s in range(0, len(points) if len(b) else 0, 65536):  # chunks keep the [n, g] float64 temporaries small
        p = np.asarray(points[s:s + 65536], np.float64)
        dx, dy = p[:, None, 0] - b[None, :, 0], p[:, None, 1] - b[None, :, 1]
        cs, sn = np.cos(b[:, 6])[None], np.sin(b[:, 6])[None]
        lx, ly = dx * cs + dy * sn, -dx * sn + dy * cs
        dz0, dz1 = p[:, None, 2] - b[None, :, 2], p[:, None, 2] - (b[None, :, 2] + b[None, :, 5])
        out[s:s + 65536] = np.minimum(np.minimum(np.abs(np.abs(lx) - b[None, :, 3] / 2), np.abs(np.abs(ly) - b[None, :, 4] / 2)),
                                      np.minimum(np.abs(dz0), np.abs(dz1)))
    return out


def random_scene(rng, n_points, n_boxes, feat, box_dim, extent=50.0, margin=1e-4, overlap=True):
    """A scene whose points all lie at least `margin` from every box face plane (the device test is f32, the restatement f64; the rule
    of tests/test_objaug_gpu.py): boxes cluster around a few centres so that they overlap, about a third of the points are drawn
    around boxes, and every point closer than `margin` to a face plane of any box is dropped."""
    centres = rng.uniform(-extent, extent, (max(1, n_boxes // 4 if overlap else n_boxes), 2))
    boxes = np.zeros((n_boxes, box_dim), np.float32)
    c = centres[rng.integers(0, len(centres), n_boxes)] + rng.normal(0, 1.5, (n_boxes, 2))
    boxes[:, :2] = c
    boxes[:, 2] = rng.uniform(-2.0, -0.5, n_boxes)
    boxes[:, 3:6] = rng.uniform(0.5, 5.0, (n_boxes, 3))
    boxes[:, 6] = rng.uniform(-np.pi, np.pi, n_boxes)
    if box_dim == 9:
        boxes[:, 7:] = rng.normal(0, 3, (n_boxes, 2))
    pts = rng.uniform(-extent, extent, (n_points, feat)).astype(np.float32)
    pts[:, 2] = rng.uniform(-3.0, 4.0, n_points)
    if n_boxes:
        k = n_points // 3
        j = rng.integers(0, n_boxes, k)
        pts[:k, :2] = boxes[j, :2] + rng.normal(0, 1.2, (k, 2)).astype(np.float32)
        pts[:k, 2] = boxes[j, 2] + rng.uniform(-0.3, 1.0, k).astype(np.float32) * boxes[j, 5]
        pts = pts[rng.permutation(n_points)]
        pts = pts[(face_distance(pts, boxes) >= margin).all(1)]
    return pts, boxes
