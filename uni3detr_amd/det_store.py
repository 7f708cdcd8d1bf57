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

Several ranks: every rank fills its own store from its share of a testing.ShardPlan, then

    whole = gather_stores(store, plan, num_classes=C)                  # on every rank: the whole dataset, in dataset order

exchanges the packed stores (a header all-gather that carries every rank's status, then four row all-gathers) and merges them with
u3d_det_store_merge; the host reads the header and the merged cursor, nothing per scene.
"""
import torch
import torch.distributed as dist

from . import native as nv


def _messages(num_classes, errors):
    return errors or ("DetStore: detection scores must be finite", f"DetStore: labels must lie in [0, {int(num_classes)})")


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
        msg = _messages(num_classes, errors)
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


# ---- several ranks ------------------------------------------------------------------------------------------------------------------
# a rank's status in the header exchange: what keeps its store out of the merge
OK, REFUSED, UNREPAIRED, BAD_SCORE, BAD_LABEL, SCENE_COUNT, BOX_DIM, OTHER = range(8)


def _local_status(store, plan, rank, num_classes, errors):
    """-> (status, packed or None, the exception or None): store.packed() with its exceptions caught, never propagated - a rank that
    raised here while its peers entered a collective would leave them waiting"""
    try:
        packed = store.packed(num_classes, errors)
    except Exception as e:                                                  # noqa: BLE001 (whatever it is, the peers must hear of it)
        _, _, n_invalid, refused = store.cursor.tolist()
        msg = _messages(num_classes, errors)
        if refused:
            return REFUSED, None, e
        if n_invalid > len(store._put):
            return UNREPAIRED, None, e
        if isinstance(e, ValueError) and str(e) in msg:
            return (BAD_SCORE if str(e) == msg[0] else BAD_LABEL), None, e
        return OTHER, None, e
    if int(packed[3].numel()) - 1 != plan.scenes(rank):
        return SCENE_COUNT, packed, None
    return OK, packed, None


def _raise_for(heads, plan, num_classes, errors, own_rank, own_error):
    """the same exception on every rank, for the first rank whose status is not OK (heads: [(scenes, rows, status, box_dim), ...])"""
    dims = {h[3] for h in heads}
    for r, (scenes, rows, status, _) in enumerate(heads):
        if status == OK:
            continue
        msg = _messages(num_classes, errors)
        kind, text = {
            REFUSED: (RuntimeError, "appends were refused because they did not fit its store - their detections are missing"),
            UNREPAIRED: (RuntimeError, "invalid batches are still empty - put() what invalid_batches() lists before the gather"),
            BAD_SCORE: (ValueError, msg[0]),
            BAD_LABEL: (ValueError, msg[1]),
            SCENE_COUNT: (RuntimeError, f"its store holds {scenes} scenes, the plan gives it {plan.scenes(r)}"),
        }.get(status, (RuntimeError, "its packed() raised - that rank's own traceback says what"))
        raise kind(f"gather_stores: rank {r} of {len(heads)}: {text}") from (own_error if r == own_rank else None)
    if len(dims) > 1:
        raise RuntimeError(f"gather_stores: the ranks' stores differ in box_dim ({sorted(dims)})")


def exchange_stores(store, plan, group=None, num_classes=0, errors=None):
    """Steps 1 - 3 of gather_stores: -> (the shards in u3d_det_store_merge's wire form, on every rank: (sh_boxes [W, Nmax, D], sh_scores
    [W, Nmax], sh_labels int32 [W, Nmax], sh_off int32 [W, Smax + 1], sh_head int32 [W, 2]); the rows of all shards together).  Raises
    on EVERY rank, before any row moves, when one rank's store cannot be packed or does not hold the plan's scene count."""
    on = dist.is_available() and dist.is_initialized()
    W = dist.get_world_size(group) if on else 1
    rank = dist.get_rank(group) if on else 0
    if plan.world != W:
        raise ValueError(f"gather_stores: a plan for {plan.world} rank(s) in a group of {W}")
    dev, D = store.device, store.box_dim
    status, packed, err = _local_status(store, plan, rank, num_classes, errors)
    scenes, rows = (int(packed[3].numel()) - 1, int(packed[0].shape[0])) if packed is not None else (0, 0)
    head = torch.tensor([scenes, rows, status, D], dtype=torch.int32, device=dev)
    heads = torch.empty((W, 4), dtype=torch.int32, device=dev)
    if W > 1:
        dist.all_gather(list(heads.unbind(0)), head, group=group)
    else:
        heads[0].copy_(head)
    host = heads.tolist()                                                    # the header: the one host read of the exchange
    _raise_for(host, plan, num_classes, errors, rank, err)
    Nmax, Smax = max(1, max(h[1] for h in host)), max(h[0] for h in host)
    wire = []
    for src, shape in zip(packed, ((Nmax, D), (Nmax,), (Nmax,), (Smax + 1,))):
        mine = src.new_zeros(shape)                                           # padded to the group's maxima: what lies past a
        mine[:src.shape[0]].copy_(src)                                        # shard's own rows / offsets is never read by the merge
        out = src.new_empty((W,) + shape)
        if W > 1:
            dist.all_gather(list(out.unbind(0)), mine, group=group)
        else:
            out[0].copy_(mine)
        wire.append(out)
    return (*wire, heads[:, :2].contiguous()), sum(h[1] for h in host)


def merge_shards(wire, plan, max_num, row_capacity=None):
    """Step 4 of gather_stores without its check: the wire form into a new DetStore of plan.n_scenes scenes and row_capacity rows
    (None: W * Nmax, which needs no host read) - u3d_det_store_merge, two launches."""
    sh_boxes, sh_scores, sh_labels, sh_off, sh_head = wire
    W, Nmax, D = sh_boxes.shape
    dev = sh_boxes.device
    out = DetStore(max(plan.n_scenes, 1), max_num, D, dev, row_capacity=max(W * Nmax if row_capacity is None else int(row_capacity), 1),
                   invalid_capacity=0)
    scene_map = torch.from_numpy(plan.scene_map()).to(dev)
    nv.det_store_merge(sh_boxes, sh_scores, sh_labels, sh_off, sh_head, scene_map, out.boxes, out.scores, out.labels, out.table,
                       out.cursor, out.invalid)
    return out


def gather_stores(store, plan, group=None, num_classes=0, errors=None):
    """Called by every rank of `group` after its own testing.test_dataset over plan.order(rank): -> a new DetStore, on every rank, that
    holds the whole dataset in dataset order; packed / results / len and the evaluators' add_store take it as any other, its
    invalid_batches() is empty.  num_classes / errors: as packed() takes them - the check runs on every rank's own rows, before the
    exchange.  A rank whose store has refused appends, unrepaired invalid batches, a non-finite score, a label out of range or another
    scene count than plan.scenes(rank) makes EVERY rank raise (RuntimeError, or ValueError for the score / label checks) with that
    rank's number and the cause, after the header exchange and before any row collective: no rank is left waiting in one.  Works over
    nccl (RCCL, one GPU per rank) and over gloo with device tensors; world 1 or no initialised process group takes the same path
    without collectives.  Host reads: the header and the merged cursor."""
    wire, total = exchange_stores(store, plan, group, num_classes, errors)
    out = merge_shards(wire, plan, store.max_num, row_capacity=total)
    scenes, rows, _, refused = out.cursor.tolist()
    if refused or scenes != plan.n_scenes:
        raise RuntimeError(f"gather_stores: u3d_det_store_merge refused the shards (heads {wire[4].tolist()}, {plan.n_scenes} scenes "
                           f"mapped, {scenes} merged) - the exchanged offsets do not describe them")
    return out
