"""Input handling shared by the indoor, KITTI and nuScenes evaluators (evaluation.py, kitti_eval.py, nuscenes_eval.py): unwrapping one
`simple_test` result, the two validity questions, counts -> offsets, and the buffer that collects a dataset's detections.

Nothing here computes a metric.  Every evaluator states its own dtypes (the indoor paths work on float32 boxes, the KITTI and nuScenes
host paths on float64, their device paths on float32 and float64) and its own messages; this module only applies them in one place.
"""
import logging

import numpy as np
import torch


def to_numpy(x):
    if hasattr(x, "tensor"):
        x = x.tensor
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def print_log(msg, logger=None):
    if logger is None:
        print(msg)
    elif isinstance(logger, logging.Logger):
        logger.info(msg)
    elif logger == "silent":
        pass
    elif isinstance(logger, str):
        logging.getLogger(logger).info(msg)
    else:
        raise TypeError(f"logger should be a logging.Logger, a str or None, got {type(logger)}")


def default_device(device):
    if device is None:
        return torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
    return torch.device(device)


def offsets(counts, device=None):
    """Per-scene counts -> CSR offsets int32 [S+1]: a NumPy array, or a tensor on `device` when one is given."""
    off = np.zeros(len(counts) + 1, np.int32)
    off[1:] = np.cumsum(counts)
    return off if device is None else torch.as_tensor(off, device=device)


# --------------------------------------------------------------------------------------------------
# one result -> (boxes, scores, labels)
# --------------------------------------------------------------------------------------------------
def as_tensor(x, dtype, device):
    """arrays, sequences, tensors and box structures (`.tensor`) alike; what is no tensor goes through NumPy, so a float64 input (a
    list of Python floats included) reaches a float64 target unrounded"""
    if hasattr(x, "tensor"):
        x = x.tensor
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.asarray(x))
    return x.detach().to(device, dtype)


_NP = {torch.float32: np.float32, torch.float64: np.float64, torch.int32: np.int32, torch.int64: np.int64}


def _zeros(like, shape):
    return np.zeros(shape, like.dtype) if isinstance(like, np.ndarray) else like.new_zeros(shape)


def fit_columns(boxes, box_dim, short=None):
    """Boxes [n, k], a tensor or a NumPy array (any n; anything empty is a scene without detections) -> [n, box_dim].  Columns past
    box_dim are cut; missing ones are zero-filled (a 6-column indoor box has yaw 0), or raise ValueError(short) when `short` is given."""
    if not (boxes.size if isinstance(boxes, np.ndarray) else boxes.numel()):
        return _zeros(boxes, (0, box_dim))
    boxes = boxes.reshape(boxes.shape[0], -1)
    k = boxes.shape[1]
    if k >= box_dim:
        return boxes[:, :box_dim]
    if short is not None:
        raise ValueError(short)
    pad = _zeros(boxes, (boxes.shape[0], box_dim - k))
    return np.concatenate([boxes, pad], 1) if isinstance(boxes, np.ndarray) else torch.cat([boxes, pad], 1)


def unwrap(result, box_dim, dtype, device, short=None, result_name="pts_bbox", label_dtype=torch.int32):
    """One scene of `simple_test` output -> (boxes `dtype` [n, box_dim], scores `dtype` [n], labels `label_dtype` [n]): tensors on
    `device`, and NumPy arrays of the same types for "cpu" - per scene, NumPy costs a fraction of what small tensor operations do, and
    the host paths read NumPy anyway.  result: a dict with boxes_3d / scores_3d / labels_3d, possibly under `result_name`, or the
    (boxes, scores, labels) triple of `get_bboxes`; boxes may be a box structure with `.tensor`.  Columns: see fit_columns."""
    if isinstance(result, dict):
        result = result.get(result_name, result)
        result = (result["boxes_3d"], result["scores_3d"], result["labels_3d"])
    boxes, scores, labels = result
    if torch.device(device).type == "cpu":
        conv = lambda x, dt: to_numpy(x).astype(_NP[dt], copy=False)         # noqa: E731
    else:
        conv = lambda x, dt: as_tensor(x, dt, device)                        # noqa: E731
    return fit_columns(conv(boxes, dtype), box_dim, short), conv(scores, dtype).reshape(-1), conv(labels, label_dtype).reshape(-1)


# --------------------------------------------------------------------------------------------------
# validity: -> (a score is not finite, a label is negative, a label is >= num_classes)
# --------------------------------------------------------------------------------------------------
def invalid_host(scores, labels, num_classes=None):
    """NumPy arrays; labels: one array or a tuple of them (detections and GT); num_classes None: no upper bound."""
    labels = labels if isinstance(labels, tuple) else (labels,)
    return (not np.all(np.isfinite(scores)), any(bool(l.size and l.min() < 0) for l in labels),
            num_classes is not None and any(bool(l.size and l.max() >= num_classes) for l in labels))


def invalid_device(scores, labels, num_classes):
    """The same question on device tensors, answered with one host read."""
    labels = labels if isinstance(labels, tuple) else (labels,)
    flags = [(~torch.isfinite(scores)).any()] + [(l < 0).any() for l in labels] + [(l >= num_classes).any() for l in labels]
    flags = torch.stack(flags).cpu().tolist()                              # the one validation sync
    return flags[0], any(flags[1:1 + len(labels)]), any(flags[1 + len(labels):])


def raise_invalid(flags, errors):
    """errors: an evaluator's (score message, label message)"""
    if flags[0]:
        raise ValueError(errors[0])
    if flags[1] or flags[2]:
        raise ValueError(errors[1])


# --------------------------------------------------------------------------------------------------
# the detections of everything added so far
# --------------------------------------------------------------------------------------------------
class DetBuffer:
    """The detections an evaluator has been given, in the order they came: per add one tensor each of boxes [., box_dim], scores and
    labels on `device` (on "cpu": NumPy arrays, which cat() hands over as host tensors without a copy) and the per-scene counts.
    cat() is their concatenation, so any batching of the same scenes - one add() per scene, one add_packed() of a whole store, or a
    mix - gives the same tensors.

    The owner sets the dtypes: `dtype` for boxes and scores; labels are int32 on a device (what the kernels read) and int64 on the host.
    short: the ValueError message for boxes with fewer than box_dim columns (None: zero-fill them).  cap / cap_message: an optional
    limit on the detections of one scene, raised by add() and add_packed() alike; cap_message is formatted with n and cap."""

    def __init__(self, box_dim, dtype, device, short=None, result_name="pts_bbox", cap=None, cap_message=None):
        self.box_dim, self.dtype, self.device = int(box_dim), dtype, torch.device(device)
        self.label_dtype = torch.int64 if self.device.type == "cpu" else torch.int32
        self.short, self.result_name, self.cap, self.cap_message = short, result_name, cap, cap_message
        self.reset()

    def reset(self):
        self._boxes, self._scores, self._labels = [], [], []
        self.counts = []                                                    # detections per scene

    def __len__(self):
        return len(self.counts)

    def _append(self, boxes, scores, labels, counts):
        if self.cap is not None:
            for n in counts:
                if n > self.cap:
                    raise ValueError(self.cap_message.format(n=n, cap=self.cap))
        self._boxes.append(boxes)
        self._scores.append(scores)
        self._labels.append(labels)
        self.counts.extend(counts)

    def add(self, result):
        """one scene (see unwrap)"""
        boxes, scores, labels = unwrap(result, self.box_dim, self.dtype, self.device, self.short, self.result_name, self.label_dtype)
        self._append(boxes, scores, labels, [int(boxes.shape[0])])

    def add_packed(self, boxes, scores, labels, off):
        """a whole det_store.DetStore.packed(): rows [N, >= box_dim], scores [N], labels [N], offsets [S+1] (one host read of them)"""
        counts = torch.diff(off).tolist()
        assert sum(counts) == boxes.shape[0]
        if counts:
            self._append(*unwrap((boxes, scores, labels), self.box_dim, self.dtype, self.device, self.short, None, self.label_dtype), counts)

    def add_store(self, store, expected, mismatch, num_classes, errors):
        """Every scene of a det_store.DetStore, in its scene order: store.packed() on a device (the rows never leave it),
        store.results() into a host buffer.  num_classes / errors: the store's own check (its packed()).  ValueError(mismatch, formatted
        with n = the store's scene count) unless the store holds `expected` scenes; nothing is added then."""
        if self.device.type == "cpu":
            results = store.results(num_classes, errors)
            n = len(results)
        else:
            packed = store.packed(num_classes, errors)
            n = int(packed[3].numel()) - 1
        if n != expected:
            raise ValueError(mismatch.format(n=n))
        if self.device.type == "cpu":
            for r in results:
                self.add(r)
        else:
            self.add_packed(*packed)

    def cat(self):
        """-> contiguous tensors (boxes [N, box_dim], scores [N], labels [N], offsets int32 [S+1]) on the buffer's device"""
        if self.device.type == "cpu":
            one = lambda xs, shape, dt: torch.from_numpy(np.concatenate(xs) if xs else np.zeros(shape, _NP[dt]))  # noqa: E731
        else:
            one = lambda xs, shape, dt: torch.cat(xs) if xs else torch.zeros(shape, dtype=dt, device=self.device)  # noqa: E731
        return (one(self._boxes, (0, self.box_dim), self.dtype), one(self._scores, (0,), self.dtype),
                one(self._labels, (0,), self.label_dtype), offsets(self.counts, self.device))
