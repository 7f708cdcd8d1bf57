"""test_dataset: run a captured inference step over a dataset and collect every detection on the device (the
loop of the reference's extra_tools/test.py -> single_gpu_test, without its per-batch copy of the results to the host).

    store = DetStore(scene_capacity=len(dataset), max_num=K, box_dim=7, device="cuda")
    with BatchFeeder(samples, order, pipe, batch_size=B, drop_last=False) as feeder:
        test_dataset(step, feeder, store, reload=lambda i: scenes_of_batch(i))
    evaluator.add_store(store, gt_boxes, gt_labels); metrics = evaluator.compute()

Per batch: on_batch(i), step.run(batch), store.append(step.det, n_live=step.n_live, valid=step.valid) - for a packed dict no host read
follows, the replays queue up behind each other.  After the loop the batches whose replay was invalid (store.invalid_batches(), one
host read) are run again eagerly and exact-size and put into their places.

Test-time augmentation: a step built with views=A > 1 takes the expanded dicts a BatchFeeder yields when its pipeline carries
MultiScaleFlipAug3D (B * A scenes, tta_views, tta_params); the loop and the store count SAMPLES, the merged DetBatch of a replay is
what goes into the store - build it with max_num = the step's tta_max_num - and the repair runs inf.aug_test_batched.

Several ranks: ShardPlan deals the one-device loop's batches out round robin, every rank runs test_dataset
on its share into its own store, and det_store.gather_stores merges the stores on the device, in dataset order, on every rank:

    plan = ShardPlan(len(samples), B, world)
    store = DetStore(max(plan.scenes(rank), 1), K, 7, "cuda")
    with BatchFeeder(samples, plan.order(rank), pipe, batch_size=B, drop_last=False) as feeder:
        test_dataset(step, feeder, store, reload=..., on_batch=seed_by_global_batch, batch_ids=plan.batch_ids(rank))
    whole = gather_stores(store, plan, num_classes=C); evaluator.add_store(whole, gt_boxes, gt_labels)
"""
import numpy as np


class ShardPlan:
    """Which rank runs which batch of a dataset of n_scenes in batches of batch_size.  Global batch j - dataset positions j * B ..
    min((j + 1) * B, n) - 1, exactly the one-device loop's batch j - goes to rank j % world as that rank's local batch j // world.  Only
    the globally last batch can be partial, and it is the last local batch of its rank, so a rank's scenes number contiguously in
    its own store.  A rank without batches (world > number of batches) is legal: zero scenes.  Pure host code."""

    def __init__(self, n_scenes, batch_size, world):
        n, B, W = int(n_scenes), int(batch_size), int(world)
        if n < 0 or B < 1 or W < 1:
            raise ValueError(f"ShardPlan(n_scenes={n}, batch_size={B}, world={W}): n_scenes >= 0, batch_size and world >= 1")
        self.n_scenes, self.batch_size, self.world = n, B, W
        self.n_batches = -(-n // B)

    def _rank(self, rank):
        r = int(rank)
        if not 0 <= r < self.world:
            raise ValueError(f"ShardPlan: rank {r} of a world of {self.world}")
        return r

    def batch_ids(self, rank):
        """-> the global index of each local batch of `rank`, in local order"""
        return list(range(self._rank(rank), self.n_batches, self.world))

    def order(self, rank, order=None):
        """-> the rank's sample order for BatchFeeder(..., drop_last=False): the entries of `order` (default: 0 .. n_scenes - 1, the
        dataset positions themselves) at the positions of its batches"""
        B, n = self.batch_size, self.n_scenes
        if order is not None:
            order = list(order)
            if len(order) != n:
                raise ValueError(f"ShardPlan.order: an order of {len(order)} entries for {n} scenes")
        pos = [p for j in self.batch_ids(rank) for p in range(j * B, min((j + 1) * B, n))]
        return pos if order is None else [order[p] for p in pos]

    def scenes(self, rank):
        """-> how many scenes `rank` runs"""
        B, n = self.batch_size, self.n_scenes
        return sum(min((j + 1) * B, n) - j * B for j in self.batch_ids(rank))

    def scene_map(self):
        """-> int32 [n_scenes, 2]: (shard, local scene) of every dataset position - u3d_det_store_merge's scene_map"""
        B, W = self.batch_size, self.world
        pos = np.arange(self.n_scenes, dtype=np.int64)
        j = pos // B
        return np.stack([j % W, (j // W) * B + pos % B], 1).astype(np.int32)


def _scenes(batch):
    """a batch as the list of per-scene point tensors"""
    if isinstance(batch, dict):
        from .datapath import unpack_batch
        return list(unpack_batch({k: batch[k] for k in ("points", "scene_off", "count") if k in batch})[0])
    return list(batch)


def _views_of(batch, views):
    """a batch of a step with views > 1 -> (the list of its views, their tta_params rows): run()'s list form"""
    if isinstance(batch, dict):
        return _scenes(batch), batch["tta_params"]
    if isinstance(batch, tuple) and len(batch) == 2 and not hasattr(batch[0], "shape"):
        return list(batch[0]), batch[1]
    raise ValueError(f"test_dataset: with views = {views} a batch is the expanded packed dict or the pair (list of views, tta_params)")


def test_dataset(step, batches, store, reload=None, on_batch=None, batch_ids=None):
    """step: a captured inference.InferenceStep; batches: any iterable of what step.run takes (a feeder.BatchFeeder yields packed dicts;
    a last dict with fewer scenes than the step's batch goes through run's list form, which pads and gates - that one batch costs a
    host read; a list holds 1 .. B scenes, as run() demands); store: a det_store.DetStore with room for the dataset - its
    scene count is read once before the loop, so that a store which already holds an earlier part works.
    A step with views = A > 1 (test-time augmentation): a dict holds B * A scenes, view-minor, and counts (scenes // A) samples; a partial
    last dict goes through the list form together with its tta_params rows; a list batch is the pair (list of n * A views, tta_params
    [n * A, 9]).  The store receives one merged scene per sample, so it is built with max_num = the step's tta_max_num: a step whose
    `det` is wider than store.max_num raises ValueError.  reload(i) returns the expanded dict or that pair; the repair runs
    step.inf.aug_test_batched.
    on_batch(i): called before batch i runs, and again before its repair - the head draws random query points in every eval forward,
    so a caller who wants reproducible results seeds there.
    reload(i): returns the scenes of batch i again (a list of point tensors or a packed dict) for the repair of an invalid replay - the
    loop keeps no batch, a feeder's slots are reused.  Each repaired batch is counted in step.fallbacks; an invalid batch without
    `reload` raises RuntimeError.
    batch_ids: the global index of every batch of this loop (ShardPlan.batch_ids(rank)) - on_batch and reload then receive batch_ids[i]
    in place of i, and the messages name that batch, so that a rank seeds and reloads by the batch's place in the dataset as the
    one-device loop does.  None: the loop's own count.  -> store."""
    gid = (lambda i: i) if batch_ids is None else (lambda i: batch_ids[i])
    A = int(getattr(step, "views", 1))
    base = first = len(store)            # (a host read before anything is in flight) a store may already hold an earlier part
    starts = {}
    for i, batch in enumerate(batches):
        tab = None
        if isinstance(batch, dict):
            n = (int(batch["scene_off"].numel()) - 1) // A
            if n < step.batch_size:
                batch, tab = _views_of(batch, A) if A > 1 else (_scenes(batch), None)
        elif A > 1:
            batch, tab = _views_of(batch, A)
            n = len(batch) // A
        else:
            batch = list(batch)
            n = len(batch)
        if on_batch is not None:
            on_batch(gid(i))
        if tab is None:
            step.run(batch)
        else:
            step.run(batch, tta_params=tab)
        width, room = getattr(getattr(step.det, "boxes", None), "shape", None), getattr(store, "max_num", None)
        if width is not None and room is not None and int(width[1]) > int(room):
            raise ValueError(f"test_dataset: the step's detections are {int(width[1])} rows wide, the store was built for max_num = {room}"
                             + (" - build it with max_num = the step's tta_max_num" if A > 1 else ""))
        store.append(step.det, n_live=step.n_live, valid=step.valid)
        starts[first] = (i, n)
        first += n
    for scene, n in store.invalid_batches():
        if scene < base:
            continue                     # an earlier loop's, repaired there
        if starts.get(scene, (None, None))[1] != n:
            raise RuntimeError(f"test_dataset: the store reports an invalid batch of scenes {scene} .. {scene + n - 1} that this loop did "
                               "not append")
        i = gid(starts[scene][0])
        if reload is None:
            raise RuntimeError(f"test_dataset: the replay of batch {i} (scenes {scene} .. {scene + n - 1}) was invalid (a sparse level "
                               "over its capacity, an FPS time-out or a scene cut to point_capacity) and no reload= was given to run it again")
        again = reload(i)
        if A > 1:
            scenes, tab = _views_of(again, A)
            if len(scenes) != n * A:
                raise RuntimeError(f"test_dataset: reload({i}) returned {len(scenes)} views = {len(scenes) / A:g} samples of {A} views, "
                                   f"batch {i} had {n} samples")
        else:
            scenes = _scenes(again)
            if len(scenes) != n:
                raise RuntimeError(f"test_dataset: reload({i}) returned {len(scenes)} scenes, batch {i} had {n}")
        if on_batch is not None:
            on_batch(i)
        if A > 1:
            det = step.inf.aug_test_batched(scenes, tta_params=tab, views=A, box_type_3d=step.box_type_3d, on_device=True,
                                            nms_thr=step.tta_nms_thr, max_num=step.tta_max_num)
        else:
            det = step.inf.simple_test_batched(None, scenes, on_device=True)
        store.put(scene, det)
        step.fallbacks += 1
    return store


test_dataset.__test__ = False        # a library function: not for pytest to collect where a test module imports it
