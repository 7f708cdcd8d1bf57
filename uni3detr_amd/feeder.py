"""BatchFeeder: a two-slot prefetcher between a dataset's files and the captured steps.

    feeder = BatchFeeder(samples, order, pipe, batch_size=B, depth=2, device="cuda", box_type_3d="Depth", drop_last=True)
    with feeder:
        for batch in feeder:               # batch i+1 is read, uploaded and transformed while batch i runs
            ts.set_packed_batch(batch); ts.step()          # or step.run(batch)

samples[k] = dict(pts_filename, gt_bboxes_3d=np [g, 7|9] | None, gt_labels_3d=np | None, info=<get_data_info dict, for sweeps> | None);
order: any iterable of sample indices (shuffling, RepeatDataset, CBGS stay with the caller); pipe: a DevicePipeline built with
load=True (with sweeps=True the feeder reads the sweep files too).

Who does what.  ONE reader thread does file reads only (datapath.read_points, and read_sweeps with the choices it is handed): it
never calls into torch.cuda or the HIP runtime.  Every GPU enqueue happens on the consumer's thread inside __next__ - the pinned
upload (datapath.pack_batch(None, ..., raw=...)), then pipe(...), both on one side stream the feeder owns - and so does every random
draw, in batch order: the sweep choice of batch k + 1 is drawn right after the pipeline of batch k has made its draws, which is the
order of the synchronous loop `pipe(pack_batch(None, ..., raw=..., sweeps=...))`.  A feeder started from a given np.random state
therefore yields bit-identical batches.  (The reader can for that reason run only one batch ahead of the enqueue when sweeps are
read; without sweeps it runs depth - 1 ahead.)

__next__: the current stream waits on the returned batch's event; every tensor of the batch gets record_stream(current) (they were
allocated on the side stream); the next batch is enqueued if its read is complete (else the following __next__ waits for it); return.
Pinned staging: `depth` slots, used in turn; a slot is rewritten only after the upload that last used it has completed (an event,
checked on the consumer's thread).  A reader exception is re-raised from __next__; close() / context exit stops and joins the reader.
"""
import queue
import threading

import numpy as np
import torch

from . import datapath as dp


def _tensors(x):
    if torch.is_tensor(x):
        yield x
    elif isinstance(x, dict):
        for v in x.values():
            yield from _tensors(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            yield from _tensors(v)


class BatchFeeder:
    def __init__(self, samples, order, pipe, batch_size, depth=2, device="cuda", box_type_3d="Depth", drop_last=True, load_cfg=None,
                 sweeps_cfg=None, pack=None):
        """load_cfg / sweeps_cfg: the loading entries (default: pipe.load_cfg / pipe.sweeps_cfg); pack: what turns the records of a
        batch into the packed dict (default: datapath.pack_batch) - with device="cpu" and a pack / pipe of the caller's the feeder
        runs without a GPU (no stream, no event, no pinned slot), which is how its ordering and shutdown are tested."""
        if int(depth) < 2:
            raise ValueError("BatchFeeder: depth >= 2 (one batch in use, one in flight)")
        if int(batch_size) < 1:
            raise ValueError("BatchFeeder: batch_size >= 1")
        self.samples, self.pipe, self.batch_size, self.depth = samples, pipe, int(batch_size), int(depth)
        self.device, self.box_type_3d, self.drop_last = torch.device(device), box_type_3d, bool(drop_last)
        self.load_cfg = load_cfg if load_cfg is not None else getattr(pipe, "load_cfg", None)
        self.sweeps_cfg = sweeps_cfg if sweeps_cfg is not None else getattr(pipe, "sweeps_cfg", None)
        if self.load_cfg is None:
            raise ValueError("BatchFeeder needs a pipeline with the device loader (DevicePipeline(..., load=True))")
        self._sweep_entry = dp.OBJECT_AUG.build(dict(self.sweeps_cfg)) if self.sweeps_cfg is not None else None
        self._pack = pack if pack is not None else dp.pack_batch
        self._order = iter(order)
        self._gpu = self.device.type == "cuda"
        self._tasks, self._results = queue.Queue(), queue.Queue()
        self._stop = threading.Event()
        self._pending = 0              # read tasks posted and not yet taken
        self._exhausted = False
        self._ready = None             # (batch, event) enqueued ahead
        self._stream = None
        self._slots = [None] * self.depth
        self._slot_events = [None] * self.depth
        self._slot = 0
        self._ahead = 1 if self._sweep_entry is not None else self.depth - 1
        self._reader = threading.Thread(target=self._read_loop, name="u3d-batch-reader", daemon=True)
        self._reader.start()

    # ---- the reader thread: file reads only -------------------------------------------------------------------------------
    def _read_loop(self):
        while not self._stop.is_set():
            try:
                task = self._tasks.get(timeout=0.1)
            except queue.Empty:
                continue
            if task is None:
                return
            idx, choices = task
            try:
                recs = [dp.read_points(self.samples[k], self.load_cfg) for k in idx]
                sw = None
                if choices is not None:
                    sw = [dp.read_sweeps(self.samples[k]["info"], self.sweeps_cfg, choices=c) for k, c in zip(idx, choices)]
                self._results.put((idx, recs, sw, None))
            except BaseException as e:          # noqa: BLE001 - handed to the consumer, which re-raises it
                self._results.put((idx, None, None, e))

    # ---- the consumer's thread ------------------------------------------------------------------------------------------
    def _post(self):
        """hand the reader the next batches of the order, with their sweep choices drawn here"""
        while not self._exhausted and self._pending < self._ahead:
            idx = []
            for k in self._order:
                idx.append(int(k))
                if len(idx) == self.batch_size:
                    break
            if len(idx) < self.batch_size:
                self._exhausted = True
                if not idx or self.drop_last:
                    return
            choices = None
            if self._sweep_entry is not None:
                e, choices = self._sweep_entry, []
                for k in idx:
                    n = len(self.samples[k]["info"]["sweeps"])
                    choices.append(np.zeros(0, np.int64) if e.pad_empty_sweeps and n == 0 else e.choose(n, np.random))
            self._tasks.put((idx, choices))
            self._pending += 1

    def _pinned(self, nbytes):
        s = self._slot
        if self._slot_events[s] is not None:
            self._slot_events[s].synchronize()          # the upload that last used this slot (long done in steady state)
        if self._slots[s] is None or self._slots[s].numel() < nbytes:
            self._slots[s] = torch.empty((int(nbytes * 1.25) + 4096,), dtype=torch.uint8, pin_memory=True)
        return self._slots[s]

    def _enqueue(self, block):
        """take the next finished read, upload and transform it on the side stream -> True when a batch is now enqueued ahead"""
        if self._pending == 0:
            self._post()
            if self._pending == 0:
                return False
        try:
            idx, recs, sw, err = self._results.get(block=block)
        except queue.Empty:
            return False
        self._pending -= 1
        if err is not None:
            self.close()
            raise err
        gts = [self.samples[k].get("gt_bboxes_3d") for k in idx]
        labs = [self.samples[k].get("gt_labels_3d") for k in idx]
        gts = None if any(g is None for g in gts) else gts
        labs = None if gts is None or any(l is None for l in labs) else labs
        kw = dict(raw=recs, device=self.device)
        if sw is not None:
            kw["sweeps"] = sw
        if self._gpu:
            if self._stream is None:
                self._stream = torch.cuda.Stream(self.device)
                self._stream.wait_stream(torch.cuda.current_stream(self.device))      # once: what the pipeline holds (database, seeds)
            with torch.cuda.stream(self._stream):
                batch = self._pack(None, gts, self.box_type_3d, gt_labels_3d=labs, pinned=self._pinned, **kw)
                up = torch.cuda.Event()
                up.record(self._stream)
                self._slot_events[self._slot] = up
                self._slot = (self._slot + 1) % self.depth
                batch = self.pipe(batch)
                ev = torch.cuda.Event()
                ev.record(self._stream)
        else:
            batch, ev = self.pipe(self._pack(None, gts, self.box_type_3d, gt_labels_3d=labs, **kw)), None
        self._ready = (batch, ev)
        self._post()
        return True

    def __iter__(self):
        return self

    def __next__(self):
        if self._stop.is_set():
            raise StopIteration
        if self._ready is None and not self._enqueue(block=True):
            raise StopIteration
        batch, ev = self._ready
        self._ready = None
        if ev is not None:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)
            for t in _tensors(batch):
                if t.is_cuda:
                    t.record_stream(cur)
        self._enqueue(block=False)
        return batch

    def close(self):
        self._stop.set()
        self._tasks.put(None)
        if self._reader.is_alive() and threading.current_thread() is not self._reader:
            self._reader.join(timeout=5.0)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
