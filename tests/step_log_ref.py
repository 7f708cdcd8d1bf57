"""Plain numpy restatement of the step log (include/u3d_hip.h: u3d_step_log_append / u3d_step_log_window): a ring of uint32 words and
a python-int cursor.  Used by tests/test_step_log_cpu.py and tests/test_step_log_gpu.py, which compare the kernels with it bit for bit."""
import numpy as np

FIXED = 8
ACCUMULATED, APPLIED, DROPPED, HELD = 0, 1, 2, 3


def _bits(x):
    return np.array([x], dtype=np.float32).view(np.uint32)[0]


class StepLogRef:
    def __init__(self, capacity, n_terms):
        self.capacity, self.n_terms, self.cols = int(capacity), int(n_terms), FIXED + int(n_terms)
        self.ring = np.zeros((self.capacity, self.cols), np.uint32)
        self.cursor = 0

    def append(self, terms, total, opt_state, acc_state=None):
        """terms: n_terms floats; total: a float; opt_state: 16 floats; acc_state: 8 floats or None."""
        st = np.asarray(opt_state, np.float32)
        acc = None if acc_state is None else np.asarray(acc_state, np.float32)
        row = np.zeros(self.cols, np.uint32)
        row[0] = np.array([self.cursor], dtype=np.int64).astype(np.int32).view(np.uint32)[0]
        row[1] = np.uint32(int(acc[5]) if acc is not None else (HELD if st[11] > 0 else APPLIED))
        row[2] = _bits(total)
        row[3] = _bits(acc[6] if acc is not None else st[4])
        row[4], row[5], row[6], row[7] = _bits(st[1]), _bits(st[5]), _bits(st[6]), 0
        row[FIXED:] = np.asarray(terms, np.float32).view(np.uint32)
        self.ring[self.cursor % self.capacity] = row
        self.cursor += 1

    def window(self, last):
        """-> (out f32 [cols, 4] = mean, min, max, rows used; counts int32 [4] = rows seen, held, dropped, non-finite totals)."""
        n = max(0, min(int(last), self.cursor, self.capacity))
        rows = [self.ring[k % self.capacity] for k in range(self.cursor - n, self.cursor)]        # ascending step order
        out = np.zeros((self.cols, 4), np.float32)
        counts = np.zeros(4, np.int32)
        counts[0] = n
        counts[1] = sum(int(r[1]) == HELD for r in rows)
        counts[2] = sum(int(r[1]) == DROPPED for r in rows)
        for c in range(2, self.cols):
            s, lo, hi, used = np.float64(0), np.float32(0), np.float32(0), 0
            for r in rows:
                o = int(r[1])
                if o == HELD:
                    continue
                v = r[c:c + 1].view(np.float32)[0]
                if not np.isfinite(v):
                    counts[3] += c == 2
                    continue
                if c in (3, 4) and o != APPLIED:
                    continue
                s = s + np.float64(v)
                lo = v if not used else min(lo, v)
                hi = v if not used else max(hi, v)
                used += 1
            out[c] = (np.float32(s / np.float64(used)) if used else 0, lo, hi, used)
        return out, counts
