"""DetStore: the detections of a whole dataset on the device (csrc/det_store.hip).

    store = DetStore(scene_capacity=len(dataset), max_num=K, box_dim=7, device="cuda")
    store.append(step.det, n_live=step.n_live, valid=step.valid)      # after every step.run(): two launches, no host read
    for first, n in store.invalid_batches():                           # replays the validity gate emptied (one host read)
        store.put(first, eager_detections_of_those_scenes)
    boxes, scores, labels, det_off = store.packed()                    # the evaluators' flat layout, scenes in dataset order
    evaluator.add_store(store, ...)                                    # IndoorEvaluator / KittiEvaluator / NuScenesEvaluator

The buffers (`boxes` [R, D], `scores` [R], `labels` int32 [R], `table` int32 [S, 2], `cursor` int32 [4], `invalid` int32 [M, 2]) live on
the device and the cursor moves there: include/u3d_hip.h states what u3d_det_store_append / u3d_det_store_pack do with them.  An append
that does not fit is refused as a whole on the device and counted; nothing is truncated, and packed() raises for it.  What the host
keeps is only which invalid ranges were reported and which of them were put.  GPU only, as the rest of the library is.
"""
import torch

from . import native as nv


class DetStore:
    def __init__(self, scene_capacity, max_num, box_dim, device, row_capacity=None, invalid_capacity=1024):
        """row_capacity defaults to scene_capacity * max_num: with it the rows cannot overflow before the scenes do, because a scene
        holds at most max_num rows and an invalid scene holds none until its repair."""
        S, K, D, M = int(scene_capacity), int(max_num), int(box_dim), int(invalid_capacity)
        R = S * K if row_capacity is None else int(row_capacity)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"DetStore lives on a GPU, not on {dev}")
        if S < 1 or R < 1 or M < 0 or not 1 <= K <= nv.DET_TAIL_MAX_K or D not in (7, 9):
            raise ValueError(f"DetStore(scene_capacity={S}, max_num={K} of at most {nv.DET_TAIL_MAX_K}, box_dim={D}, row_capacity={R}, "
                             f"invalid_capacity={M}): capacities >= 1, box_dim 7 or 9")
        if R * D >= 2 ** 31:
            raise ValueError(f"DetStore: row_capacity * box_dim = {R * D} must stay below 2^31 - pass a row_capacity sized to the "
                             "detections the dataset really yields")
        self.scene_capacity, self.max_num, self.box_dim, self.row_capacity, self.invalid_capacity = S, K, D, R, M
        self.device = dev
        self.boxes = torch.empty((R, D), dtype=torch.float32, device=dev)         # never read at or past the used rows
        self.scores = torch.empty((R,), dtype=torch.float32, device=dev)
        self.labels = torch.empty((R,), dtype=torch.int32, device=dev)
        self.table = torch.empty((S, 2), dtype=torch.int32, device=dev)
        self.invalid = torch.empty((M, 2), dtype=torch.int32, device=dev)
        self.cursor = torch.zeros((4,), dtype=torch.int32, device=dev)
        self._reported, self._put = [], set()

    def reset(self):
        """Empty the store (stream-ordered; the buffers stay)."""
        self.cursor.zero_()
        self._reported, self._put = [], set()

    # ---- filling ----------------------------------------------------------------------------------------------------------
    def _check_det(self, det):
        if det.boxes.dim() != 3 or int(det.boxes.shape[2]) != self.box_dim:
            raise ValueError(f"DetStore: boxes of shape {tuple(det.boxes.shape)} do not go into a store of box_dim {self.box_dim}")
        if det.boxes.device != self.device:
            raise ValueError(f"DetStore: the detections live on {det.boxes.device}, the store on {self.device}")

    def append(self, det, n_live=None, valid=None):
        """The leading n_live scenes of a native.DetBatch become the next scenes of the store (n_live, valid: device int32 [1] or None =
        all of them / valid).  No host read, no allocation, no synchronisation; capturable.  An invalid batch is recorded as empty
        scenes and listed by invalid_batches()."""
        self._check_det(det)
        nv.det_store_append(det, n_live, valid, None, self.boxes, self.scores, self.labels, self.table, self.cursor, self.invalid)

    def invalid_batches(self):
        """-> [(first scene, number of scenes), ...] of the appends whose `valid` was 0, in order.  One host read."""
        n = int(self.cursor[2])
        if n > self.invalid_capacity:
            raise RuntimeError(f"DetStore: {n} invalid batches were counted but invalid_capacity = {self.invalid_capacity} of them are "
                               "listed - build the store with a larger invalid_capacity (or capture the step with larger margins)")
        self._reported = [tuple(r) for r in self.invalid[:n].tolist()] if n else []
        return list(self._reported)

    def put(self, first_scene, dets):
        """The repair of an invalid range: `dets` = one (boxes [n, D], scores [n], labels [n]) per scene, or a native.DetBatch of those
        scenes.  ValueError unless (first_scene, len(dets)) was reported by invalid_batches() and has not been put yet."""
        key = (int(first_scene), len(dets))
        if key not in self._reported:
            self.invalid_batches()
        if key not in self._reported:
            raise ValueError(f"DetStore.put: scenes {key[0]} .. {key[0] + key[1] - 1} were not reported as one invalid batch "
                             f"(reported: {self._reported})")
        if key in self._put:
            raise ValueError(f"DetStore.put: scenes {key[0]} .. {key[0] + key[1] - 1} have been put already")
        if not isinstance(dets, nv.DetBatch):
            most = max(int(d[1].shape[0]) for d in dets)
            if most > self.max_num:
                raise ValueError(f"DetStore.put: a scene with {most} detections, the store was built for max_num = {self.max_num}")
            dets = nv.DetBatch.from_list(dets, self.max_num, self.box_dim, self.device)
        self._check_det(dets)
        ids = torch.arange(key[0], key[0] + key[1], dtype=torch.int32, device=self.device)
        nv.det_store_append(dets, None, None, ids, self.boxes, self.scores, self.labels, self.table, self.cursor, self.invalid)
        self._put.add(key)

    # ---- reading ------------------------------------------------------------------------------------------------------------
    def _state(self):
        """(scenes, rows) after the one host read of the cursor; raises for refused appends and unrepaired invalid batches"""
        scenes, rows, n_invalid, refused = self.cursor.tolist()
        if refused:
            raise RuntimeError(f"DetStore: {refused} append(s) were refused because they did not fit (scene_capacity = "
                               f"{self.scene_capacity}, row_capacity = {self.row_capacity}; {scenes} scenes and {rows} rows are in use) - "
                               "their detections are not in the store")
        if n_invalid > len(self._put):
            raise RuntimeError(f"DetStore: {n_invalid - len(self._put)} of {n_invalid} invalid batch(es) are still empty - put() what "
                               "invalid_batches() lists first")
        return scenes, rows

    def __len__(self):
        """Scenes recorded so far.  One host read."""
        return int(self.cursor[0])

    def packed(self, num_classes=0, errors=None):
        """-> (boxes [N, D], scores [N], labels int32 [N], det_off int32 [S + 1]) on the device, scenes in the order they were appended:
        what native.eval_* and the evaluators take.  One host read of the cursor before the pack, one of its two flags and det_off[-1]
        after it.  RuntimeError for refused appends or unrepaired invalid batches; ValueError (errors = the two messages, an
        evaluator's own) for a non-finite score or, with num_classes > 0, a label outside [0, num_classes).  N = det_off[-1]: through
        append / put that is the cursor's row count (put is refused for a range that holds rows); rows orphaned by a direct
        native.det_store_append(..., scene_ids) on these buffers are left out."""
        scenes, rows = self._state()
        boxes, scores, labels, off, bad = nv.det_store_pack(self.boxes, self.scores, self.labels, self.table, scenes, rows, num_classes)
        bad_score, bad_label, n = torch.cat([bad, off[-1:]]).tolist()
        msg = errors or ("DetStore: detection scores must be finite", f"DetStore: labels must lie in [0, {int(num_classes)})")
        if bad_score:
            raise ValueError(msg[0])
        if bad_label:
            raise ValueError(msg[1])
        if n > rows:
            raise RuntimeError(f"DetStore: the table references {n} rows but {rows} are in use - the buffers were written from outside")
        return boxes[:n], scores[:n], labels[:n], off

    def results(self, num_classes=0, errors=None):
        """-> simple_test_batched's list of dicts on the host (boxes_3d, scores_3d, labels_3d long), one per scene: one copy per tensor
        for the whole store."""
        boxes, scores, labels, off = (t.cpu() for t in self.packed(num_classes, errors))
        off, labels = off.tolist(), labels.long()
        return [dict(boxes_3d=boxes[a:b], scores_3d=scores[a:b], labels_3d=labels[a:b]) for a, b in zip(off[:-1], off[1:])]
