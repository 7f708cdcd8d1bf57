"""Device-resident ground-truth object database for GT-paste (mmdet3d ObjectSample / the plugin's UnifiedObjectSample).

Storage (all on one device): points [P, F] f32, every object's points relative to its box's (x, y, z_bottom) as mmdet3d's
`create_groundtruth_database` writes them; obj_off int32 [D+1] (object d = points rows obj_off[d] .. obj_off[d+1]); boxes [D, 7|9] f32;
labels int32 [D] (index into `classes`).  `num_points_in_gt`, `difficulty` and host copies of obj_off / boxes stay on the host.

Per database key a host `BatchSampler` with mmdet3d's semantics (recalled, v1.0.0rc5 datasets/pipelines/dbsampler.py): a shuffled index
list (`np.random.shuffle` at construction and on every reset); `sample(num)` returns the tail and reshuffles when idx + num >= n, so it
can return fewer than num.  The samplers are built in the order of the database's keys, as UnifiedDataBaseSampler builds them
(ref: projects/mmdet3d_plugin/datasets/pipelines/dbsampler.py), so the host RNG stream follows the reference's.
"""
import os
import pickle

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
