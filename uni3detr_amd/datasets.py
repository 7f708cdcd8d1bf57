"""samples_from_cfg: a config's dataset section -> the sample list feeder.BatchFeeder takes.

    samples, meta = samples_from_cfg(cfg.data.train)
    plan = EpochPlan(len(samples), B, repeat=meta["repeat"], class_ids=meta["class_ids"])

What mmdet3d's dataset classes do between an info pickle and the pipeline's first entry, restated for the four dataset types of the
shipped point-cloud configs (mmdet3d v1.0.0rc5's SUNRGBDDataset / ScanNetDataset / KittiDataset get_data_info + get_ann_info, recalled,
parity unpinned; NuScenesSweepDataset: projects/mmdet3d_plugin/datasets/nuscenes_dataset.py).  The wrappers are unwrapped, not applied:
RepeatDataset gives meta["repeat"], CBGSDataset gives meta["class_ids"] (get_cat_ids, nuscenes_dataset.py:161-183), and
training.EpochPlan applies both to the order.

samples[k] = dict(pts_filename, gt_bboxes_3d f32 [g, 7|9] bottom-centre as plugin.structures.Boxes3D holds them, gt_labels_3d int64 [g]
(-1: a name outside `classes`, which the pipeline's ObjectNameFilter drops), info = what datapath.read_sweeps takes | None).
meta: kind, classes, box_type_3d, repeat, class_ids | None, infos (the info dicts of the kept samples, in order: what KittiEvaluator /
NuScenesEvaluator.add_store take), gt_boxes / gt_labels (indoor: gravity-centre rows and labels per sample, what
IndoorEvaluator.add_store takes).

filter_empty_gt (training sets only, as upstream): a sample without a box of a known class is left out of the list - upstream draws
another random sample in its place each time it meets one; with a static list the epoch is shorter by those samples instead.
Info files are read by gtdb.load_info_file: a restricted unpickler, `trusted=True` for files that hold more than arrays.
"""
import os

import numpy as np

from . import gtdb

SUNRGBD_CLASSES = ("bed", "table", "sofa", "chair", "toilet", "desk", "dresser", "night_stand", "bookshelf", "bathtub")
SCANNET_CLASSES = ("cabinet", "bed", "chair", "sofa", "table", "door", "window", "bookshelf", "picture", "counter", "desk", "curtain",
                   "refrigerator", "showercurtrain", "toilet", "sink", "bathtub", "garbagebin")
DEFAULT_CLASSES = dict(SUNRGBDDataset=SUNRGBD_CLASSES, ScanNetDataset=SCANNET_CLASSES, KittiDataset=("car", "pedestrian", "cyclist"),
                       NuScenesSweepDataset=("car", "truck", "trailer", "bus", "construction_vehicle", "bicycle", "motorcycle", "pedestrian",
                                             "traffic_cone", "barrier"))
KINDS = dict(SUNRGBDDataset="indoor", ScanNetDataset="indoor", KittiDataset="kitti", NuScenesSweepDataset="nuscenes")


def _join(root, path):
    return path if root is None or os.path.isabs(path) else os.path.join(root, path)


def _labels(names, classes):
    where = {c: i for i, c in enumerate(classes)}
    return np.asarray([where.get(str(n), -1) for n in names], np.int64)


def _indoor(info, cfg, classes):
    a = info.get("annos") or {}
    n = int(a.get("gt_num", 0))
    if n:
        raw = np.asarray(a["gt_boxes_upright_depth"], np.float32).reshape(n, -1)
        grav = np.zeros((n, 7), np.float32)
        grav[:, :raw.shape[1]] = raw[:, :7]            # (ScanNet boxes have no yaw column: 0)
        labels = np.asarray(a["class"], np.int64).reshape(n)
        if "name" in a and tuple(classes) != tuple(DEFAULT_CLASSES[cfg["type"]]):
            labels = _labels(a["name"], classes)       # a `classes` subset re-numbers the labels by name
    else:
        grav, labels = np.zeros((0, 7), np.float32), np.zeros((0,), np.int64)
    bottom = grav.copy()
    bottom[:, 2] += bottom[:, 5] * np.float32(-0.5)    # gravity centre -> bottom centre (DepthInstance3DBoxes origin (.5, .5, .5))
    sample = dict(pts_filename=_join(cfg.get("data_root"), info["pts_path"]), gt_bboxes_3d=bottom, gt_labels_3d=labels, info=None)
    return sample, labels, dict(gt_boxes=grav, gt_labels=labels)


def _kitti(info, cfg, classes):
    root = cfg.get("data_root")
    s = gtdb.kitti_scene(info, root or "")
    labels = _labels(s["gt_names"], classes)
    if cfg.get("split") is not None and cfg.get("pts_prefix") is not None:       # KittiDataset._get_pts_filename
        path = os.path.join(root or "", cfg["split"], cfg["pts_prefix"], f"{int(info['image']['image_idx']):06d}.bin")
    else:
        path = s["points_path"]
    return dict(pts_filename=path, gt_bboxes_3d=s["gt_bboxes_3d"], gt_labels_3d=labels, info=None), labels, {}


def _nuscenes(info, cfg, classes):
    s = gtdb.nuscenes_scene(info, cfg.get("data_root") or "")
    mask = s["valid_flag"] if cfg.get("use_valid_flag", False) else np.asarray(info["num_lidar_pts"]) > 0
    boxes = s["gt_bboxes_3d"][mask]
    if not cfg.get("with_velocity", True):
        boxes = boxes[:, :7]
    labels = _labels(s["gt_names"][mask], classes)
    # get_cat_ids (nuscenes_dataset.py:161-183) looks at the valid boxes with use_valid_flag and at ALL boxes without it
    cat = labels if cfg.get("use_valid_flag", False) else _labels(s["gt_names"], classes)
    return (dict(pts_filename=s["points_path"], gt_bboxes_3d=boxes, gt_labels_3d=labels, info=s["sweeps_info"]), labels,
            dict(cat_ids=sorted(set(cat[cat >= 0].tolist()))))


_READERS = dict(indoor=_indoor, kitti=_kitti, nuscenes=_nuscenes)


def samples_from_cfg(data_cfg, trusted=False):
    """data_cfg: one split of a config's `data` section (cfg.data.train / val / test).  -> (samples, meta), see the module docstring."""
    cfg, repeat, balanced = dict(data_cfg), 1, False
    while cfg.get("type") in ("RepeatDataset", "CBGSDataset"):
        if cfg["type"] == "RepeatDataset":
            repeat *= int(cfg["times"])
        else:
            balanced = True
        cfg = dict(cfg["dataset"])
    kind = KINDS.get(cfg.get("type"))
    if kind is None:
        raise NotImplementedError(f"samples_from_cfg: dataset type {cfg.get('type')!r}; supported: {sorted(KINDS)} behind RepeatDataset / "
                                  "CBGSDataset")
    classes = tuple(cfg.get("classes") or DEFAULT_CLASSES[cfg["type"]])
    infos = gtdb.load_info_file(_join(None, cfg["ann_file"]), trusted=trusted)
    if kind == "nuscenes":
        infos = sorted(infos["infos"] if isinstance(infos, dict) else infos, key=lambda e: e["timestamp"])[::int(cfg.get("load_interval", 1))]
    test_mode = bool(cfg.get("test_mode", False))
    drop_empty = bool(cfg.get("filter_empty_gt", True)) and not test_mode
    samples, kept, class_ids, extra = [], [], [], dict(gt_boxes=[], gt_labels=[])
    for info in infos:
        sample, labels, more = _READERS[kind](info, cfg, classes)
        known = labels[labels >= 0]
        if drop_empty and known.size == 0:
            continue
        samples.append(sample)
        kept.append(info)
        class_ids.append(more.pop("cat_ids", None) or sorted(set(known.tolist())))
        for k, v in more.items():
            extra[k].append(v)
    box_type = cfg.get("box_type_3d") or ("Depth" if kind == "indoor" else "LiDAR")
    meta = dict(kind=kind, dataset=cfg["type"], classes=classes, box_type_3d=box_type, repeat=repeat, class_ids=class_ids if balanced else None,
                infos=kept, pipeline=cfg.get("pipeline"), test_mode=test_mode)
    if kind == "indoor":
        meta.update(extra)
    return samples, meta
