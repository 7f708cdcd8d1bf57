"""A NumPy restatement of u3d_det_store_append (append and the scene_ids repair path) and u3d_det_store_pack, written from the
header's text: include/u3d_hip.h is the contract, this is what the tests hold csrc/det_store.hip to."""
import numpy as np

POISON_I = -1


class RefStore:
    def __init__(self, scene_capacity, row_capacity, box_dim, invalid_capacity):
        S, R, D, M = scene_capacity, row_capacity, box_dim, invalid_capacity
        self.S, self.R, self.D, self.M = S, R, D, M
        self.boxes = np.full((R, D), np.nan, np.float32)           # the poison the GPU test pre-fills its store with
        self.scores = np.full((R,), np.nan, np.float32)
        self.labels = np.full((R,), POISON_I, np.int32)
        self.table = np.full((S, 2), POISON_I, np.int32)
        self.invalid = np.full((M, 2), POISON_I, np.int32)
        self.cursor = np.zeros(4, np.int32)

    def arrays(self):
        return dict(boxes=self.boxes, scores=self.scores, labels=self.labels, table=self.table, invalid=self.invalid, cursor=self.cursor)

    def append(self, boxes, scores, labels, count, n_live=None, valid=None, scene_ids=None):
        """boxes [B, K, D], scores / labels [B, K], count [B]; n_live / valid ints or None; scene_ids [B] or None"""
        B, K, _ = boxes.shape
        nl = B if n_live is None else min(max(int(n_live), 0), B)
        ok = True if valid is None else int(valid) != 0
        cnt = [min(max(int(c), 0), K) if ok else 0 for c in count[:nl]]
        scenes, rows = int(self.cursor[0]), int(self.cursor[1])
        if scene_ids is None:
            refuse = scenes + nl > self.S or rows + sum(cnt) > self.R
        else:
            refuse = rows + sum(cnt) > self.R or not ok or any(not 0 <= int(s) < scenes for s in scene_ids[:nl])
        if refuse:
            self.cursor[3] += 1
            return False
        for b in range(nl):
            c = cnt[b]
            self.boxes[rows:rows + c], self.scores[rows:rows + c], self.labels[rows:rows + c] = boxes[b, :c], scores[b, :c], labels[b, :c]
            self.table[scenes + b if scene_ids is None else int(scene_ids[b])] = (rows, c)      # in order of b: a repeated id, the last wins
            rows += c
        self.cursor[1] = rows
        if scene_ids is None:
            self.cursor[0] = scenes + nl
            if not ok and nl > 0:
                if self.cursor[2] < self.M:
                    self.invalid[self.cursor[2]] = (scenes, nl)
                self.cursor[2] += 1
        return True

    def pack(self, n_scenes=None, num_classes=0):
        """-> boxes [N, D], scores [N], labels [N], off [n_scenes + 1], bad [2]"""
        n = int(self.cursor[0]) if n_scenes is None else n_scenes
        runs = [(int(f), int(c)) for f, c in self.table[:n]]
        take = np.concatenate([np.arange(f, f + c) for f, c in runs] + [np.zeros(0, np.int64)]).astype(np.int64)
        off = np.concatenate([[0], np.cumsum([c for _, c in runs])]).astype(np.int32)
        sc, lb = self.scores[take], self.labels[take]
        bad = np.array([int(not np.all(np.isfinite(sc))), int(num_classes > 0 and bool(((lb < 0) | (lb >= num_classes)).any()))], np.int32)
        return self.boxes[take], sc, lb, off, bad


def random_det(rng, B, K, D, counts=None):
    """A DetBatch as NumPy arrays: rows past count[b] are zero; without `counts`, 0 and K occur in every draw (B >= 3)."""
    if counts is None:
        counts = rng.permutation([0, K] + [int(rng.integers(0, K + 1)) for _ in range(B - 2)])
    count = np.asarray(counts, np.int32)
    live = np.arange(K)[None, :] < count[:, None]
    boxes = (rng.normal(0, 3, (B, K, D)) * live[..., None]).astype(np.float32)
    scores = (rng.uniform(0.1, 1, (B, K)) * live).astype(np.float32)
    labels = (rng.integers(0, 3, (B, K)) * live).astype(np.int32)
    return boxes, scores, labels, count


def concat_lists(per_scene, D):
    """The plain statement of what a store must hold: per scene (boxes [n, D], scores [n], labels [n]) -> flat arrays and offsets."""
    boxes = np.concatenate([p[0] for p in per_scene] + [np.zeros((0, D), np.float32)])
    scores = np.concatenate([p[1] for p in per_scene] + [np.zeros(0, np.float32)])
    labels = np.concatenate([p[2] for p in per_scene] + [np.zeros(0, np.int32)])
    off = np.concatenate([[0], np.cumsum([p[1].shape[0] for p in per_scene])]).astype(np.int32)
    return boxes.astype(np.float32), scores.astype(np.float32), labels.astype(np.int32), off
