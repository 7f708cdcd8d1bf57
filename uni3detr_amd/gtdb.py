"""Device-resident ground-truth object database for GT-paste (mmdet3d ObjectSample / the plugin's UnifiedObjectSample).

Storage (all on one device): points [P, F] f32, every object's points relative to its box's (x, y, z_bottom) as mmdet3d's
`create_groundtruth_database` writes them; obj_off int32 [D+1] (object d = points rows obj_off[d] .. obj_off[d+1]); boxes [D, 7|9] f32;
labels int32 [D] (index into `classes`).  `num_points_in_gt`, `difficulty` and host copies of obj_off / boxes stay on the host.

Per database key a host `BatchSampler` with mmdet3d's semantics (recalled, v1.0.0rc5 datasets/pipelines/dbsampler.py): a shuffled index
list (`np.random.shuffle` at construction and on every reset); `sample(num)` returns the tail and reshuffles when idx + num >= n, so it
can return fewer than num.  The samplers are built in the order of the database's keys, as UnifiedDataBaseSampler builds them
(ref: projects/mmdet3d_plugin/datasets/pipelines/dbsampler.py), so the host RNG stream follows the reference's.

Building the database: `create_groundtruth_database` (the counterpart of the reference's
extra_tools/data_converter/create_unified_gt_database.py, camera branch left out) walks a data set in chunks of scenes, crops every
object on the device (csrc/gtdb.hip), and writes mmdet3d's `dbinfos` pickle with per-object .bin files and / or one packed .npz.
`python -m uni3detr_amd.gtdb --help` is the command line over mmdet3d-style KITTI / nuScenes info pickles.
"""
import argparse
import io
import os
import pickle
import sys

import numpy as np
import torch

from . import native as nv


class BatchSampler:
    """mmdet3d BatchSampler (recalled): indices into a list of `n` entries."""

    def __init__(self, n, name=None, shuffle=True):
        self._indices = np.arange(n)
        if shuffle:
            np.random.shuffle(self._indices)
        self._idx, self._example_num, self._name, self._shuffle = 0, n, name, shuffle

    def _reset(self):
        if self._shuffle:
            np.random.shuffle(self._indices)
        self._idx = 0

    def sample(self, num):
        if self._idx + num >= self._example_num:
            ret = self._indices[self._idx:].copy()
            self._reset()
        else:
            ret = self._indices[self._idx:self._idx + num]
            self._idx += num
        return ret


def filter_by_difficulty(db_infos, removed_difficulty):
    """ref: UnifiedDataBaseSampler.filter_by_difficulty."""
    return {k: [i for i in v if i["difficulty"] not in removed_difficulty] for k, v in db_infos.items()}


def filter_by_min_points(db_infos, min_gt_points_dict):
    """ref: UnifiedDataBaseSampler.filter_by_min_points (filters the named keys in place, keeps the rest)."""
    for name, min_num in min_gt_points_dict.items():
        min_num = int(min_num)
        if min_num > 0:
            db_infos[name] = [i for i in db_infos[name] if i["num_points_in_gt"] >= min_num]
    return db_infos


_PREPARE = {"filter_by_difficulty": filter_by_difficulty, "filter_by_min_points": filter_by_min_points}


class GTDatabase:
    def __init__(self, classes, names, points, obj_off, boxes, labels, num_points_in_gt, difficulty, key_sizes):
        """Use from_infos / from_scenes.  names[d] = database key of object d; key_sizes: (key, n) for every key, in database order -
        the samplers draw indices into the key's own list, which is the objects of that key in database order."""
        self.classes = list(classes)
        self.points, self.obj_off, self.boxes, self.labels = points, obj_off, boxes, labels
        self.obj_off_host = obj_off.cpu().numpy()
        self.boxes_host = boxes.cpu().numpy()
        self.num_points_in_gt = np.asarray(num_points_in_gt, np.int64)
        self.difficulty = np.asarray(difficulty, np.int64)
        self.box_dim = int(boxes.shape[1])
        self.feat = int(points.shape[1])
        names = np.asarray(names, dtype=object)
        self.rows = {k: np.nonzero(names == k)[0].astype(np.int64) for k, _ in key_sizes}
        self.samplers = {k: BatchSampler(n, k, shuffle=True) for k, n in key_sizes}

    def __len__(self):
        return int(self.boxes.shape[0])

    def sample(self, name, num):
        """`num` database rows of class `name` (possibly fewer: BatchSampler's tail)."""
        return self.rows[name][self.samplers[name].sample(num)]

    @classmethod
    def from_infos(cls, info_path, data_root, classes, prepare, points_loader=None, device="cuda"):
        """An mmdet3d `*_dbinfos_train.pkl` (plain pickle: {class name: [info dict]}) and the .bin files it names; `prepare` as in the
        config's db_sampler, applied in its order; points_loader's load_dim / use_dim as in the config (default 4 / [0, 1, 2, 3])."""
        with open(info_path, "rb") as f:
            db_infos = pickle.load(f)
        for fn, val in (prepare or {}).items():
            db_infos = _PREPARE[fn](db_infos, val)
        pl = points_loader or {}
        load_dim = int(pl.get("load_dim", 4))
        use_dim = pl.get("use_dim", [0, 1, 2, 3])
        use_dim = list(range(use_dim)) if isinstance(use_dim, int) else list(use_dim)
        cat = {n: i for i, n in enumerate(classes)}
        names, pts, off, boxes, labels, npts, diff = [], [], [0], [], [], [], []
        for key, infos in db_infos.items():
            for info in infos:
                path = os.path.join(data_root, info["path"]) if data_root else info["path"]
                p = np.fromfile(path, dtype=np.float32).reshape(-1, load_dim)[:, use_dim]
                names.append(key)
                pts.append(p)
                off.append(off[-1] + p.shape[0])
                boxes.append(np.asarray(info["box3d_lidar"], np.float32))
                labels.append(cat.get(key, -1))
                npts.append(int(info["num_points_in_gt"]))
                diff.append(int(info["difficulty"]))
        feat = len(use_dim)
        dim = boxes[0].shape[0] if boxes else 7
        return cls(classes, names, *_upload(pts, off, boxes, labels, feat, dim, device), npts, diff,
                   [(k, len(v)) for k, v in db_infos.items()])

    @classmethod
    def from_packed(cls, path, classes, prepare=None, device="cuda"):
        """The .npz create_groundtruth_database(packed_path=...) wrote; `prepare` as in from_infos (filter_by_difficulty,
        filter_by_min_points, in the config's order).  Labels follow `classes` (a key outside it gets -1), as in from_infos."""
        with np.load(path, allow_pickle=False) as z:
            d = {k: z[k] for k in z.files}
        missing = [k for k in PACKED_FIELDS if k not in d]
        if missing:
            raise ValueError(f"{path}: not a packed GT database (missing {missing})")
        db_infos = {k: [] for k in dict.fromkeys(str(n) for n in d["names"])}          # key-major: first appearance is the key order
        for i, n in enumerate(d["names"]):
            db_infos[str(n)].append(dict(row=i, difficulty=int(d["difficulty"][i]), num_points_in_gt=int(d["num_points"][i])))
        for fn, val in (prepare or {}).items():
            db_infos = _PREPARE[fn](db_infos, val)
        order = np.asarray([i["row"] for v in db_infos.values() for i in v], np.int64)
        dev = torch.device(device)
        pts, off = _gather_objects(torch.from_numpy(d["points"].astype(np.float32)).to(dev), d["obj_off"], order)
        cat = {n: i for i, n in enumerate(classes)}
        names = [k for k, v in db_infos.items() for _ in v]
        return cls(classes, names, pts.contiguous(), off, torch.from_numpy(d["boxes"][order].astype(np.float32)).to(dev).contiguous(),
                   torch.tensor(np.asarray([cat.get(k, -1) for k in names], np.int32), device=dev), d["num_points"][order], d["difficulty"][order],
                   [(k, len(v)) for k, v in db_infos.items()])

    @classmethod
    def from_scenes(cls, points, boxes, labels, classes):
        """The counterpart of create_groundtruth_database for scenes already on the device: lists of per-scene points [n, F], boxes
        [g, 7|9] (bottom-centre) and labels [g] (index into `classes`).  Every box becomes one object holding the scene points strictly
        inside it (the points-in-box kernel), relative to its (x, y, z_bottom); difficulty 0.  Objects keep scene order; the database
        keys are `classes` in order."""
        dev = points[0].device
        from .datapath import pack_batch
        batch = pack_batch(points, boxes, "LiDAR", gt_labels_3d=labels)
        P, G = batch["points"], batch["gt_bboxes_3d"]
        so, go = batch["scene_off"], batch["gt_off"]
        maxn = max(int(p.shape[0]) for p in points)
        maxg = max(int(b.shape[0]) for b in boxes)
        _, bits, _ = nv.points_in_boxes(P, so, None, maxn, G, go, max_boxes=maxg, want_bits=True)
        so_h, go_h = so.cpu().numpy(), go.cpu().numpy()
        objs = []
        for b in range(len(points)):
            n, g = so_h[b + 1] - so_h[b], go_h[b + 1] - go_h[b]
            if g == 0 or n == 0:
                objs += [P.new_zeros((0, P.shape[1]))] * g
                continue
            w = bits[so_h[b]:so_h[b + 1]]
            for j in range(g):
                sel = ((w[:, j // 32] >> (j % 32)) & 1).bool()
                o = P[so_h[b]:so_h[b + 1]][sel].clone()
                o[:, :3] -= G[go_h[b] + j, :3]
                objs.append(o)
        lab = torch.cat([l.to(torch.int32) for l in labels]).to(dev) if G.shape[0] else torch.zeros((0,), dtype=torch.int32, device=dev)
        lab_h = lab.cpu().numpy()
        names = [classes[int(l)] for l in lab_h]
        sizes = [int(o.shape[0]) for o in objs]
        off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), device=dev)
        pts = torch.cat(objs).contiguous() if objs else P.new_zeros((0, P.shape[1]))
        return cls(classes, names, pts, off, G.clone(), lab.contiguous(), sizes, np.zeros(len(sizes)),
                   [(c, int(np.sum(lab_h == i))) for i, c in enumerate(classes)])


def _upload(pts, off, boxes, labels, feat, dim, device):
    dev = torch.device(device)
    p = torch.from_numpy(np.concatenate(pts).astype(np.float32) if pts else np.zeros((0, feat), np.float32)).to(dev).contiguous()
    o = torch.tensor(np.asarray(off, np.int32), device=dev)
    b = torch.from_numpy(np.stack(boxes).astype(np.float32) if boxes else np.zeros((0, dim), np.float32)).to(dev).contiguous()
    l = torch.tensor(np.asarray(labels, np.int32), device=dev)
    return p, o, b, l


# --------------------------------------------------------------------------------------------------
# Building the database (ref: extra_tools/data_converter/create_unified_gt_database.py, the camera branch left out)
# --------------------------------------------------------------------------------------------------
# the reference script's NuScenesSweepDataset pipeline entry (create_unified_gt_database.py:59-63)
SWEEPS_ENTRY = dict(type="LoadPointsFromMultiSweeps", sweeps_num=10, load_dim=5, use_dim=[0, 1, 2, 3, 4], pad_empty_sweeps=True,
                    remove_close=True)
PACKED_FIELDS = ("points", "obj_off", "boxes", "labels", "names", "num_points", "difficulty", "group_id", "classes")


def _host(x, dtype=None):
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return a if dtype is None else a.astype(dtype, copy=False)


class DbInfoBuilder:
    """The bookkeeping of the reference's loop (create_unified_gt_database.py:85-176) without the geometry: which boxes of a scene
    become database objects (`select`) and, once their point counts are known, their info dicts (`add`).  Host only."""

    def __init__(self, info_prefix, used_classes=None):
        self.info_prefix = info_prefix
        self.used_classes = None if used_classes is None else set(used_classes)
        self.db_infos, self.group_counter = {}, 0
        self.order = []                                    # (key, index within the key's list) per object, in data-set order

    def select(self, scene):
        """-> (boxes f32 [g, 7|9] of the scene after the valid flag, gt_idx int64 [k] of those that become objects).  The valid flag
        is applied first, as NuScenesSweepDataset(use_valid_flag=True) applies it before the script sees the boxes: a dropped box
        takes no gt_idx.  used_classes drops objects but does not renumber gt_idx."""
        boxes = _host(scene["gt_bboxes_3d"], np.float32)
        boxes = boxes.reshape(-1, boxes.shape[-1] if boxes.ndim == 2 else 7)
        if boxes.shape[1] not in (7, 9):
            raise ValueError(f"gt_bboxes_3d has {boxes.shape[1]} columns (7 or 9: bottom-centre x, y, z, dx, dy, dz, yaw [, vx, vy])")
        names = np.asarray(scene["gt_names"]).reshape(-1)
        if len(names) != len(boxes):
            raise ValueError(f"sample {scene['sample_idx']!r}: {len(boxes)} boxes and {len(names)} names")
        mask = np.ones(len(boxes), bool) if scene.get("valid_flag") is None else _host(scene["valid_flag"]).astype(bool).reshape(-1)
        meta = dict(sample_idx=scene["sample_idx"], boxes=boxes[mask], names=names[mask])
        for k in ("difficulty", "group_ids", "score"):
            meta[k] = None if scene.get(k) is None else _host(scene[k]).reshape(-1)[mask]
        used = self.used_classes
        meta["gt_idx"] = np.asarray([i for i, n in enumerate(meta["names"]) if used is None or n in used], np.int64)
        return meta

    def add(self, meta, num_points):
        """num_points [k]: the point counts of the scene's objects, in gt_idx order."""
        group_dict = {}
        for i, n_pts in zip(meta["gt_idx"], num_points):
            name = str(meta["names"][i])
            file = f"{meta['sample_idx']}_{name}_{int(i)}.bin"
            info = dict(name=name, path=os.path.join(f"{self.info_prefix}_gt_database", "pts_dir", file), image_idx=meta["sample_idx"],
                        image_path="", image_crop_key="", image_crop_depth=0, gt_idx=int(i), box3d_lidar=meta["boxes"][i].copy(),
                        num_points_in_gt=int(n_pts), difficulty=np.int32(0) if meta["difficulty"] is None else meta["difficulty"][i])
            local = int(i) if meta["group_ids"] is None else meta["group_ids"][i].item()
            if local not in group_dict:
                group_dict[local] = self.group_counter
                self.group_counter += 1
            info["group_id"] = group_dict[local]
            if meta["score"] is not None:
                info["score"] = meta["score"][i]
            self.db_infos.setdefault(name, []).append(info)
            self.order.append((name, len(self.db_infos[name]) - 1))

    def key_major(self):
        """-> int64 [D]: the data-set-order index of every object, key after key (the order from_infos builds from the pickle)."""
        first = {}
        for k in self.db_infos:
            first[k] = len(first)
        rank = np.asarray([first[k] for k, _ in self.order], np.int64)
        return np.argsort(rank, kind="stable")


def _crop_chunk(scenes, metas, device):
    """One chunk on the device: upload, sweep merge where a scene brings its sweeps record, crop -> (points [P, F], obj_off [D+1],
    num_points [D]) device tensors; object order = scene after scene, gt_idx order."""
    from . import datapath as dp
    dev = torch.device(device)
    if dev.type != "cuda":
        raise nv.U3DError("create_groundtruth_database crops on the GPU (csrc/gtdb.hip); there is no host path")
    pts = [s["points"] for s in scenes]
    lens = [int(p.shape[0]) for p in pts]
    if all(not isinstance(p, torch.Tensor) or not p.is_cuda for p in pts):
        feat = int(pts[0].shape[1])
        P = torch.from_numpy(np.ascontiguousarray(np.concatenate([_host(p, np.float32).reshape(-1, feat) for p in pts]))).to(dev)
    else:
        P = torch.cat([p.to(dev, torch.float32) if isinstance(p, torch.Tensor) else torch.from_numpy(_host(p, np.float32)).to(dev)
                       for p in pts]).contiguous()
    recs = [s.get("sweeps") for s in scenes]
    max_rows = max(lens)
    if any(r is not None for r in recs):
        if any(r is None for r in recs):
            raise ValueError("a chunk mixes scenes with and without a sweeps record")
        entry = dp.OBJECT_AUG.build(dict(SWEEPS_ENTRY))
        off = np.concatenate([[0], np.cumsum(lens)])
        batch = dp.pack_batch([P[off[b]:off[b + 1]] for b in range(len(lens))], box_type_3d="LiDAR", sweeps=recs)
        batch = entry(batch)
        P, scene_off = batch["points"].contiguous(), batch["scene_off"]
        max_rows = max(n * (1 + r["sweeps_num"]) if r["pad"] else n + sum(len(a) for a in r["points"]) for n, r in zip(lens, recs))
    else:
        scene_off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), device=dev)
    sel = [m["boxes"][m["gt_idx"]] for m in metas]
    dim = sel[0].shape[1]
    if any(b.shape[1] != dim for b in sel):
        raise ValueError("boxes of 7 and of 9 columns in one data set")
    B = torch.from_numpy(np.ascontiguousarray(np.concatenate(sel))).to(dev)
    box_off = torch.tensor(np.concatenate([[0], np.cumsum([len(b) for b in sel])]).astype(np.int32), device=dev)
    return nv.gtdb_crop(P, scene_off, None, max_rows, B, box_off, max_boxes=max(len(b) for b in sel))


def write_dbinfos(db_infos, out_dir, info_prefix):
    path = os.path.join(out_dir, f"{info_prefix}_dbinfos_train.pkl")
    os.makedirs(out_dir, exist_ok=True)
    with open(path, "wb") as f:
        pickle.dump(db_infos, f)
    return path


def write_object_points(out_dir, infos, points, obj_off):
    """infos[d]['path'] under out_dir <- points[obj_off[d]:obj_off[d+1]] as raw float32 rows (what upstream mmdet3d writes)."""
    points, obj_off = _host(points, np.float32), _host(obj_off)
    made = set()
    for d, info in enumerate(infos):
        path = os.path.join(out_dir, info["path"])
        if os.path.dirname(path) not in made:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            made.add(os.path.dirname(path))
        points[obj_off[d]:obj_off[d + 1]].tofile(path)


def write_packed(path, db_infos, classes, points, obj_off):
    """ONE .npz holding the whole database, key-major (points / obj_off in the order of db_infos' keys and lists); read by
    GTDatabase.from_packed without any pickle."""
    flat = [(k, i) for k, v in db_infos.items() for i in v]
    cat = {n: i for i, n in enumerate(classes)}
    dim = flat[0][1]["box3d_lidar"].shape[0] if flat else 7
    points = _host(points, np.float32)
    np.savez(path, points=points, obj_off=_host(obj_off, np.int32),
             boxes=np.stack([i["box3d_lidar"] for _, i in flat]).astype(np.float32) if flat else np.zeros((0, dim), np.float32),
             labels=np.asarray([cat.get(k, -1) for k, _ in flat], np.int32), names=np.asarray([k for k, _ in flat], dtype=str),
             num_points=np.asarray([i["num_points_in_gt"] for _, i in flat], np.int64),
             difficulty=np.asarray([i["difficulty"] for _, i in flat], np.int64),
             group_id=np.asarray([i["group_id"] for _, i in flat], np.int64), classes=np.asarray(list(classes), dtype=str))


def _database(classes, db_infos, points, obj_off, device):
    flat = [(k, i) for k, v in db_infos.items() for i in v]
    cat = {n: i for i, n in enumerate(classes)}
    dim = flat[0][1]["box3d_lidar"].shape[0] if flat else 7
    dev = torch.device(device)
    boxes = torch.from_numpy(np.stack([i["box3d_lidar"] for _, i in flat]).astype(np.float32) if flat else np.zeros((0, dim), np.float32))
    labels = torch.tensor(np.asarray([cat.get(k, -1) for k, _ in flat], np.int32))
    return GTDatabase(classes, [k for k, _ in flat], points.to(dev).contiguous(), obj_off.to(dev, torch.int32), boxes.to(dev), labels.to(dev),
                      [i["num_points_in_gt"] for _, i in flat], [i["difficulty"] for _, i in flat], [(k, len(v)) for k, v in db_infos.items()])


def _gather_objects(points, obj_off, order):
    """objects re-ordered by `order` (host int64 [D']) with one gather -> (points, obj_off int32 [D'+1]) on points' device."""
    off = _host(obj_off).astype(np.int64)
    sizes = (off[1:] - off[:-1])[order]
    new_off = np.concatenate([[0], np.cumsum(sizes)])
    rows = np.repeat(off[:-1][order] - new_off[:-1], sizes) + np.arange(new_off[-1])
    idx = torch.from_numpy(rows).to(points.device)
    return points.index_select(0, idx), torch.from_numpy(new_off.astype(np.int32)).to(points.device)


def create_groundtruth_database(scenes, classes, *, info_prefix, used_classes=None, out_dir=None, write_points=False, packed_path=None,
                                chunk_scenes=8, device="cuda", return_database=True):
    """The reference's create_groundtruth_database (extra_tools/data_converter/create_unified_gt_database.py) with the geometry on the
    device -> (db_infos, GTDatabase or None when return_database=False).

    scenes: an iterable (a generator is fine: it is walked once, `chunk_scenes` at a time) of dicts
      sample_idx, points [n, F] (numpy or tensor, host or device), gt_bboxes_3d [g, 7|9] bottom-centre LiDAR boxes, gt_names [g],
      optional difficulty / group_ids / valid_flag / score [g], optional sweeps (the record datapath.read_sweeps returns: the points are
      then the 5-column key frame and the cloud is merged on the device with the reference script's settings, SWEEPS_ENTRY).
    Every box that passes valid_flag and used_classes becomes one object: the points strictly inside it, in scene order, relative to
    the box's (x, y, z_bottom).  Only those boxes are uploaded; per chunk there is one crop (native.gtdb_crop) and one host read.

    db_infos follows the reference's schema: {class name (order of first appearance): [dict(name, path, image_idx, image_path,
    image_crop_key, image_crop_depth, gt_idx, box3d_lidar, num_points_in_gt, difficulty, group_id[, score])]}.  The camera branch is
    out of scope: image_path and image_crop_key are '' and image_crop_depth is 0, no img_dir is written.

    out_dir: the pickle goes to {out_dir}/{info_prefix}_dbinfos_train.pkl; write_points=True also writes every object's [n, F] float32
    rows to {out_dir}/{path}, which is what upstream mmdet3d does (the reference script has its `tofile` commented out and relies on
    files made earlier).  packed_path: ONE .npz of the whole database for GTDatabase.from_packed.  The returned database and the packed
    file hold the objects key-major (all of the first key in data-set order, then the next key): the order GTDatabase.from_infos
    builds from the pickle, which the host samplers index into.

    Device memory: the scene points of one chunk, plus - only when a database or a packed file is asked for - the cropped objects so
    far (a small fraction of the scene points).  With neither, nothing outlives its chunk."""
    if write_points and out_dir is None:
        raise ValueError("write_points needs out_dir")
    builder = DbInfoBuilder(info_prefix, used_classes)
    keep = return_database or packed_path is not None
    kept_pts, kept_sizes, feat = [], [], None
    chunk = []

    def flush():
        nonlocal feat
        metas = [builder.select(s) for s in chunk]
        pts, off, num = _crop_chunk(chunk, metas, device)
        feat = int(pts.shape[1])
        num_h = num.cpu().numpy()
        first = len(builder.order)
        k0 = 0
        for m in metas:
            builder.add(m, num_h[k0:k0 + len(m["gt_idx"])])
            k0 += len(m["gt_idx"])
        if write_points:
            infos = [builder.db_infos[k][i] for k, i in builder.order[first:]]
            write_object_points(out_dir, infos, pts, np.concatenate([[0], np.cumsum(num_h)]))
        if keep:
            kept_pts.append(pts)
            kept_sizes.append(num_h.astype(np.int64))
        chunk.clear()

    for s in scenes:
        chunk.append(s)
        if len(chunk) >= int(chunk_scenes):
            flush()
    if chunk:
        flush()
    db_infos = builder.db_infos
    if out_dir is not None:
        write_dbinfos(db_infos, out_dir, info_prefix)
    if not keep:
        return db_infos, None
    dev = torch.device(device)
    pts = torch.cat(kept_pts) if kept_pts else torch.zeros((0, feat or 4), dtype=torch.float32, device=dev)
    off = np.concatenate([[0], np.cumsum(np.concatenate(kept_sizes))]) if kept_sizes else np.zeros(1, np.int64)
    pts, off = _gather_objects(pts, off, builder.key_major())
    if packed_path is not None:
        write_packed(packed_path, db_infos, classes, pts, off)
    return db_infos, (_database(classes, db_infos, pts, off, device) if return_database else None)


# --------------------------------------------------------------------------------------------------
# Command line: mmdet3d-style info pickles -> scene dicts
# --------------------------------------------------------------------------------------------------
class _InfoUnpickler(pickle.Unpickler):
    """Info pickles hold dicts, lists, strings, numbers and numpy arrays; nothing else is constructed."""
    _ALLOWED = {("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"), ("numpy", "ndarray"),
                ("numpy", "dtype"), ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"),
                ("collections", "OrderedDict")}

    def find_class(self, module, name):
        if (module, name) in self._ALLOWED:
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"global {module}.{name} is not allowed in an info file")


def load_info_file(path, trusted=False):
    """An info pickle read without running what it says (a restricted unpickler: containers, numbers, strings, numpy arrays).  A file
    that holds more needs the full unpickler, which EXECUTES the file: opt in with trusted=True (--trusted) or U3D_TRUST_CHECKPOINTS=1,
    as uni3detr_amd.checkpoint does; there is no silent fall-back."""
    with open(path, "rb") as f:
        raw = f.read()
    try:
        return _InfoUnpickler(io.BytesIO(raw)).load()
    except pickle.UnpicklingError as e:
        if not (trusted or os.environ.get("U3D_TRUST_CHECKPOINTS") == "1"):
            raise RuntimeError(f"{path}: holds more than containers and numpy arrays ({e}); loading it runs the code it contains. If you "
                               "trust the file pass --trusted (or set U3D_TRUST_CHECKPOINTS=1)") from e
        return pickle.loads(raw)


def kitti_scene(info, data_root):
    """mmdet3d KittiDataset.get_data_info / get_ann_info (v1.0.0rc5, recalled) for the database builder: DontCare rows dropped, the
    camera boxes (location, dimensions (l, h, w), rotation_y) moved to the LiDAR frame with inv(R0_rect @ Tr_velo_to_cam),
    (dx, dy, dz) = (l, w, h), yaw = -rotation_y - pi / 2 wrapped into [-pi, pi)."""
    a = info["annos"]
    keep = np.asarray([n != "DontCare" for n in a["name"]], bool)
    loc, dims, ry = (np.asarray(a[k], np.float64)[keep] for k in ("location", "dimensions", "rotation_y"))
    T = np.linalg.inv(np.asarray(info["calib"]["R0_rect"], np.float64).reshape(4, 4) @
                      np.asarray(info["calib"]["Tr_velo_to_cam"], np.float64).reshape(4, 4))
    xyz = np.concatenate([loc.reshape(-1, 3), np.ones((len(loc), 1))], 1) @ T.T
    yaw = -ry - np.pi / 2
    yaw = yaw - np.floor(yaw / (2 * np.pi) + 0.5) * (2 * np.pi)
    dims = dims.reshape(-1, 3)
    boxes = np.concatenate([xyz[:, :3], dims[:, [0, 2, 1]], yaw[:, None]], 1).astype(np.float32)
    scene = dict(sample_idx=info["image"]["image_idx"], gt_bboxes_3d=boxes, gt_names=np.asarray(a["name"])[keep])
    for src, dst in (("difficulty", "difficulty"), ("group_ids", "group_ids"), ("score", "score")):
        if src in a and len(a[src]) == len(keep):
            scene[dst] = np.asarray(a[src])[keep]
    if "point_cloud" in info:
        scene["points_path"] = os.path.join(data_root, info["point_cloud"]["velodyne_path"])
    return scene


def nuscenes_scene(info, data_root, rng=np.random):
    """The reference's NuScenesSweepDataset.get_data_info / get_ann_info (projects/mmdet3d_plugin/datasets/nuscenes_dataset.py) with
    use_valid_flag=True and with_velocity=True: boxes (x, y, z_centre, dx, dy, dz, yaw) + velocity (NaN -> 0) moved to bottom-centre in
    float32; the valid flag travels with the scene and is applied by the builder.  `sweeps_info` is what datapath.read_sweeps takes."""
    boxes = np.asarray(info["gt_boxes"], np.float32).reshape(-1, 7)
    vel = np.asarray(info["gt_velocity"], np.float32).reshape(-1, 2).copy()
    vel[np.isnan(vel[:, 0])] = 0.0
    boxes = np.concatenate([boxes, vel], 1)
    boxes[:, 2] += boxes[:, 5] * np.float32(-0.5)
    path = info["lidar_path"]
    return dict(sample_idx=info["token"], gt_bboxes_3d=boxes, gt_names=np.asarray(info["gt_names"]),
                valid_flag=np.asarray(info["valid_flag"], bool), points_path=path if os.path.isabs(path) else os.path.join(data_root, path),
                sweeps_info=dict(timestamp=info["timestamp"] / 1e6, sweeps=[dict(s, data_path=s["data_path"] if os.path.isabs(s["data_path"])
                                                                                 else os.path.join(data_root, s["data_path"]))
                                                                            for s in info["sweeps"]]))


def info_scenes(infos, dataset, data_root, rng=np.random):
    """info file content -> the scene dicts create_groundtruth_database takes, clouds read with numpy one scene at a time."""
    from .datapath import read_sweeps
    if dataset == "nuscenes":
        for info in sorted(infos["infos"] if isinstance(infos, dict) else infos, key=lambda e: e["timestamp"]):
            s = nuscenes_scene(info, data_root)
            s["points"] = np.fromfile(s.pop("points_path"), dtype=np.float32).reshape(-1, 5)
            s["sweeps"] = read_sweeps(s.pop("sweeps_info"), SWEEPS_ENTRY, rng=rng)
            yield s
    elif dataset == "kitti":
        for info in infos:
            s = kitti_scene(info, data_root)
            s["points"] = np.fromfile(s.pop("points_path"), dtype=np.float32).reshape(-1, 4)
            yield s
    else:
        raise ValueError(f"dataset {dataset!r} (nuscenes or kitti)")


KITTI_CLASSES = ("Pedestrian", "Cyclist", "Car")
NUSCENES_CLASSES = ("car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
                    "traffic_cone")


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m uni3detr_amd.gtdb", description="Build the GT-paste object database on the GPU from an "
                                "mmdet3d-style info pickle (the create_data step of the reference, without its camera crops).")
    p.add_argument("--infos", required=True, help="the *_infos_train.pkl")
    p.add_argument("--data-root", required=True, help="where the info file's relative paths start; outputs go here too")
    p.add_argument("--dataset", required=True, choices=("nuscenes", "kitti"))
    p.add_argument("--extra-tag", required=True, help="the info prefix: {tag}_dbinfos_train.pkl, {tag}_gt_database/")
    p.add_argument("--used-classes", nargs="+", default=None, help="keep only these classes (default: all)")
    p.add_argument("--packed", default=None, metavar="OUT.npz", help="also write the whole database as one file (GTDatabase.from_packed)")
    p.add_argument("--write-points", action="store_true", help="write every object's points to {tag}_gt_database/pts_dir/*.bin")
    p.add_argument("--chunk-scenes", type=int, default=None, help="scenes per device chunk (default: 8 nuscenes, 32 kitti)")
    p.add_argument("--trusted", action="store_true", help="the info file may hold arbitrary pickled objects: loading it runs its code")
    a = p.parse_args(argv)
    if a.chunk_scenes is None:
        a.chunk_scenes = 8 if a.dataset == "nuscenes" else 32
    if a.chunk_scenes < 1:
        p.error("--chunk-scenes must be positive")
    return a


def main(argv=None):
    a = parse_args(argv)
    infos = load_info_file(a.infos, trusted=a.trusted)
    classes = NUSCENES_CLASSES if a.dataset == "nuscenes" else KITTI_CLASSES
    db_infos, _ = create_groundtruth_database(info_scenes(infos, a.dataset, a.data_root), classes, info_prefix=a.extra_tag,
                                              used_classes=a.used_classes, out_dir=a.data_root, write_points=a.write_points,
                                              packed_path=a.packed, chunk_scenes=a.chunk_scenes, return_database=False)
    for k, v in db_infos.items():
        print(f"load {len(v)} {k} database infos")
    return 0


if __name__ == "__main__":
    sys.exit(main())
