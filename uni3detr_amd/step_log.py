"""A device-resident log of the training step (csrc/step_log.hip).

TrainStep(log=StepLog()) ends the step's last stage with one u3d_step_log_append: a row of the step's outcome, total loss, gradient
norm, clip coefficient, lr, beta1 and every loss term goes into a ring in device memory, inside the captured graph and without a host
read.  The host reads when it prints: window(last) is one launch and one small device-to-host copy of the per-column means.

    log = StepLog(capacity=4096)
    ts = TrainStep(model, ..., log=log)
    ...ts.step() x N...
    log.window(50)      # {"loss": .., "grad_norm": .., "lr": .., "loss_cls": .., ..., "steps": 50, "held": 0, "dropped": 0, "nonfinite": 0}
    log.rows(0, 10)     # int32 bits [10, columns]; columns 2.. are floats: rows.view(np.float32)
"""
import numpy as np
import torch

from . import native as nv

STEP_LOG_FIXED = 8                  # U3D_STEP_LOG_FIXED of include/u3d_hip.h (tests/test_step_log_cpu.py compares them)
MAX_TERMS = 64
FIXED_NAMES = ("step", "outcome", "loss", "grad_norm", "clip_coef", "lr", "beta1", "reserved")
COL_STEP, COL_OUTCOME, COL_LOSS, COL_GRAD_NORM, COL_CLIP, COL_LR, COL_BETA1 = range(7)
ACCUMULATED, APPLIED, DROPPED, HELD = 0, 1, 2, 3
WINDOW_KEYS = ("steps", "held", "dropped", "nonfinite", "used")       # what window() adds to the column means


class StepLog:
    def __init__(self, capacity=4096, device="cuda"):
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError(f"StepLog(capacity={capacity}): at least one row")
        self.capacity, self.device = capacity, torch.device(device)
        self.names = None                     # the loss terms' names, fixed by the first append
        self.ring = None                      # int32 [capacity, STEP_LOG_FIXED + n_terms], allocated with the names
        self.cursor = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._res = None                      # window()'s result words: [columns * 4 floats | 4 int32 counts], one copy to the host

    # ---- device side ----------------------------------------------------------------------------------------------------
    def bind(self, names):
        """Fix the column names (the first step does it); the ring is allocated here, once: captured graphs keep its address."""
        names = [str(n) for n in names]
        if self.names is not None:
            if names != self.names:
                raise ValueError(f"StepLog: the loss terms {names} differ from the columns fixed at the first step {self.names}")
            return
        if len(names) > MAX_TERMS:
            raise ValueError(f"StepLog: {len(names)} loss terms, a row holds at most {MAX_TERMS}")
        if len(set(names)) != len(names) or set(names) & set(FIXED_NAMES + WINDOW_KEYS):
            raise ValueError(f"StepLog: the loss terms {names} must be distinct and none of {FIXED_NAMES + WINDOW_KEYS}")
        self.names = names
        cols = STEP_LOG_FIXED + len(names)
        assert nv.step_log_bytes(self.capacity, len(names)) == self.capacity * cols * 4
        self.ring = torch.zeros((self.capacity, cols), dtype=torch.int32, device=self.device)
        self._res = torch.zeros(cols * 4 + 4, dtype=torch.int32, device=self.device)

    def append(self, terms, total, opt_state, acc_state=None):
        """One row on the current stream (capturable, no host read).  terms: dict name -> device f32 scalar, in the ring's order."""
        self.bind(list(terms))
        nv.step_log_append(list(terms.values()), total, opt_state, acc_state, self.ring, self.cursor)

    def snapshot(self):
        """Device clones of (ring, cursor) for restore(): TrainStep.capture() takes its warm-up steps back out of the log with them."""
        return (None if self.ring is None else self.ring.clone(), self.cursor.clone())

    def restore(self, snap):
        ring, cursor = snap
        if self.ring is not None:
            self.ring.copy_(ring) if ring is not None else self.ring.zero_()
        self.cursor.copy_(cursor)

    # ---- host side --------------------------------------------------------------------------------------------------------
    @property
    def columns(self):
        return list(FIXED_NAMES) + list(self.names or [])

    def __len__(self):
        """Rows appended so far (a device-to-host read)."""
        return int(self.cursor.item())

    def window_stats(self, last=50):
        """(out f32 [columns, 4] = mean / min / max / rows used per column, counts int32 [4] = rows seen, held, dropped, non-finite
        totals) of the latest `last` rows: one launch, one device-to-host copy."""
        if self.ring is None:
            return np.zeros((STEP_LOG_FIXED, 4), np.float32), np.zeros(4, np.int32)
        cols = self.ring.shape[1]
        nv.step_log_window(self.ring, self.cursor, int(last), self._res[:cols * 4].view(torch.float32), self._res[cols * 4:])
        host = self._res.cpu().numpy()
        return host[:cols * 4].view(np.float32).reshape(cols, 4).copy(), host[cols * 4:].copy()

    def window(self, last=50):
        """name -> mean over the latest `last` rows (held rows and non-finite values left out; grad_norm / clip_coef over applied
        updates only), plus steps, held, dropped, nonfinite and `used` = rows behind the mean of the total loss."""
        out, counts = self.window_stats(last)
        res = {n: float(out[c, 0]) for c, n in enumerate(self.columns) if c >= 2 and n != "reserved"}
        res.update(steps=int(counts[0]), held=int(counts[1]), dropped=int(counts[2]), nonfinite=int(counts[3]),
                   used=int(out[COL_LOSS, 3]))
        return res

    def rows(self, first=0, count=None):
        """Rows first .. first + count - 1 (numbered from the first append; default: up to the newest) as int32 bits [count, columns];
        columns 2.. hold float bits (`.view(np.float32)`).  Rows that left the ring are refused."""
        n = len(self)
        first = int(first)
        count = n - first if count is None else int(count)
        if count < 0 or first < max(0, n - self.capacity) or first + count > n:
            raise IndexError(f"StepLog.rows({first}, {count}): the ring holds rows {max(0, n - self.capacity)} .. {n - 1}")
        if count == 0 or self.ring is None:
            return np.zeros((0, len(self.columns)), np.int32)
        idx = (torch.arange(first, first + count, device=self.device) % self.capacity)
        return self.ring[idx].cpu().numpy()

    def state_dict(self):
        return dict(capacity=self.capacity, names=None if self.names is None else list(self.names), cursor=len(self),
                    ring=None if self.ring is None else self.ring.cpu())

    def load_state_dict(self, sd):
        """In place (captured graphs hold the ring's and the cursor's addresses)."""
        if int(sd["capacity"]) != self.capacity:
            raise ValueError(f"StepLog: the state was saved with capacity {int(sd['capacity'])}, this log has {self.capacity}")
        if sd["names"] is not None:
            self.bind(sd["names"])
            self.ring.copy_(sd["ring"])
        elif self.ring is not None:
            self.ring.zero_()
        self.cursor.fill_(int(sd["cursor"]))
