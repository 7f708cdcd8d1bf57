"""test_dataset: run a captured inference step over a dataset and collect every detection on the device (the
loop of the reference's extra_tools/test.py -> single_gpu_test, without its per-batch copy of the results to the host).

    store = DetStore(scene_capacity=len(dataset), max_num=K, box_dim=7, device="cuda")
    with BatchFeeder(samples, order, pipe, batch_size=B, drop_last=False) as feeder:
        test_dataset(step, feeder, store, reload=lambda i: scenes_of_batch(i))
    evaluator.add_store(store, gt_boxes, gt_labels); metrics = evaluator.compute()

Per batch: on_batch(i), step.run(batch), store.append(step.det, n_live=step.n_live, valid=step.valid) - for a packed dict no host read
follows, the replays queue up behind each other.  After the loop the batches whose replay was invalid (store.invalid_batches(), one
host read) are run again eagerly and exact-size and put into their places.  One device, no aug_test.
"""


def _scenes(batch):
    """a batch as the list of per-scene point tensors"""
    if isinstance(batch, dict):
        from .datapath import unpack_batch
        return list(unpack_batch({k: batch[k] for k in ("points", "scene_off", "count") if k in batch})[0])
    return list(batch)


def test_dataset(step, batches, store, reload=None, on_batch=None):
    """step: a captured inference.InferenceStep; batches: any iterable of what step.run takes (a feeder.BatchFeeder yields packed dicts;
    a last dict with fewer scenes than the step's batch goes through run's list form, which pads and gates - that one batch costs a
    host read; a list holds 1 .. B scenes, as run() demands); store: a det_store.DetStore with room for the dataset - its
    scene count is read once before the loop, so that a store which already holds an earlier part works.
    on_batch(i): called before batch i runs, and again before its repair - the head draws random query points in every eval forward,
    so a caller who wants reproducible results seeds there.
    reload(i): returns the scenes of batch i again (a list of point tensors or a packed dict) for the repair of an invalid replay - the
    loop keeps no batch, a feeder's slots are reused.  Each repaired batch is counted in step.fallbacks; an invalid batch without
    `reload` raises RuntimeError.  -> store."""
    base = first = len(store)            # (a host read before anything is in flight) a store may already hold an earlier part
    starts = {}
    for i, batch in enumerate(batches):
        if isinstance(batch, dict):
            n = int(batch["scene_off"].numel()) - 1
            if n < step.batch_size:
                batch = _scenes(batch)
        else:
            batch = list(batch)
            n = len(batch)
        if on_batch is not None:
            on_batch(i)
        step.run(batch)
        store.append(step.det, n_live=step.n_live, valid=step.valid)
        starts[first] = (i, n)
        first += n
    for scene, n in store.invalid_batches():
        if scene < base:
            continue                     # an earlier loop's, repaired there
        if starts.get(scene, (None, None))[1] != n:
            raise RuntimeError(f"test_dataset: the store reports an invalid batch of scenes {scene} .. {scene + n - 1} that this loop did "
                               "not append")
        i = starts[scene][0]
        if reload is None:
            raise RuntimeError(f"test_dataset: the replay of batch {i} (scenes {scene} .. {scene + n - 1}) was invalid (a sparse level "
                               "over its capacity, an FPS time-out or a scene cut to point_capacity) and no reload= was given to run it again")
        scenes = _scenes(reload(i))
        if len(scenes) != n:
            raise RuntimeError(f"test_dataset: reload({i}) returned {len(scenes)} scenes, batch {i} had {n}")
        if on_batch is not None:
            on_batch(i)
        store.put(scene, step.inf.simple_test_batched(None, scenes, on_device=True))
        step.fallbacks += 1
    return store


test_dataset.__test__ = False        # a library function: not for pytest to collect where a test module imports it
