"""u3d_step_log_append / u3d_step_log_window on the device against the numpy restatement (tests/step_log_ref.py), bit for bit, at the
smallest shapes that reach every branch: every row width class, an empty tail / exactly full / wrapped ring, windows shorter than,
equal to and longer than what is stored and across the wrap, every outcome with and without acc_state, NaN / Inf values, held-only
windows, a captured append, no host synchronisation, and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import step_log_ref as R
from test_varlen_gpu import _no_host_sync
from uni3detr_amd import native as nv
from uni3detr_amd.step_log import StepLog

pytestmark = pytest.mark.gpu


class _Dev:
    """The device side of one log driven through native.step_log_*, next to its restatement."""

    def __init__(self, capacity, n_terms, dev, with_acc):
        self.ref = R.StepLogRef(capacity, n_terms)
        self.ring = torch.zeros((capacity, R.FIXED + n_terms), dtype=torch.int32, device=dev)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=dev)
        self.terms = torch.zeros(max(n_terms, 1), device=dev)
        self.total = torch.zeros((), device=dev)
        self.state = torch.zeros(16, device=dev)
        self.acc = torch.zeros(8, device=dev) if with_acc else None
        self.n_terms = n_terms
        self.out = torch.full((R.FIXED + n_terms, 4), -7.0, device=dev)
        self.counts = torch.full((4,), -7, dtype=torch.int32, device=dev)

    def append(self, terms, total, state, acc=None):
        self.ref.append(terms, total, state, acc)
        self.terms[:self.n_terms].copy_(torch.from_numpy(np.asarray(terms, np.float32)))
        self.total.fill_(float(total))
        self.state.copy_(torch.from_numpy(state))
        if acc is not None:
            self.acc.copy_(torch.from_numpy(acc))
        nv.step_log_append([self.terms[i] for i in range(self.n_terms)], self.total, self.state, self.acc, self.ring, self.cursor)

    def check_ring(self):
        assert int(self.cursor.item()) == self.ref.cursor
        assert np.array_equal(self.ring.cpu().numpy().view(np.uint32), self.ref.ring)

    def check_window(self, last):
        self.out.fill_(-7.0)
        self.counts.fill_(-7)
        nv.step_log_window(self.ring, self.cursor, last, self.out, self.counts)
        out, counts = self.out.cpu().numpy(), self.counts.cpu().numpy()
        want_out, want_counts = self.ref.window(last)
        assert np.array_equal(counts, want_counts), (last, counts, want_counts)
        assert np.array_equal(out.view(np.uint32), want_out.view(np.uint32)), (last, out, want_out)
        nv.step_log_window(self.ring, self.cursor, last, self.out, self.counts)
        assert np.array_equal(self.out.cpu().numpy().view(np.uint32), out.view(np.uint32))       # two calls, the same bytes
        return out, counts


def _row(rng, n_terms, k, outcome, with_acc, bad=None):
    """(terms, total, state, acc) of step k with the given outcome; bad: None, 'total_nan', 'total_inf', 'term_nan', 'term_inf'."""
    terms = rng.uniform(0.01, 3.0, n_terms).astype(np.float32)
    total = np.float32(terms.astype(np.float64).sum())
    if bad == "total_nan":
        total = np.float32(np.nan)
    elif bad == "total_inf":
        total = np.float32(-np.inf)
    elif bad == "term_nan":
        terms[n_terms // 2] = np.nan
    elif bad == "term_inf":
        terms[-1] = np.inf
    st = np.zeros(16, np.float32)
    st[0], st[1], st[4] = k, rng.uniform(0.1, 1.0), rng.uniform(1.0, 40.0)
    st[5], st[6], st[11] = 1e-4 * (1 + k), 0.95 - 0.01 * k, 1.0 if outcome == R.HELD else 0.0
    acc = None
    if with_acc:
        acc = np.zeros(8, np.float32)
        acc[0], acc[5], acc[6] = 2, outcome, rng.uniform(1.0, 40.0)
    return terms, total, st, acc


OUTCOMES = (R.APPLIED, R.ACCUMULATED, R.HELD, R.APPLIED, R.DROPPED, R.APPLIED)
BAD = (None, "total_nan", None, "term_inf", "total_inf", "term_nan")


@pytest.mark.parametrize("n_terms", [1, 12, 36, 64])
@pytest.mark.parametrize("appends", [3, 4, 6])
@pytest.mark.parametrize("with_acc", [False, True])
def test_append_and_window_against_the_restatement(cuda, n_terms, appends, with_acc):
    rng = np.random.RandomState(100 * n_terms + 10 * appends + with_acc)
    d = _Dev(4, n_terms, cuda, with_acc)
    d.check_window(4)                                         # an empty log: zeros, no division
    for k in range(appends):
        o = OUTCOMES[k]
        if not with_acc and o in (R.ACCUMULATED, R.DROPPED):  # (without acc_state a row is applied or held)
            o = R.APPLIED
        d.append(*_row(rng, n_terms, k, o, with_acc, BAD[k]))
    d.check_ring()
    assert d.ring[:, 1].cpu().tolist() == [int(r) for r in d.ref.ring[:, 1]]
    for last in (0, 1, 2, 3, 4, 5, 50):                       # shorter than / equal to / longer than what is stored; 3+ spans the wrap at 6
        out, counts = d.check_window(last)
        assert counts[0] == min(last, appends, 4)
    out, counts = d.check_window(50)
    assert counts[1] == sum(int(r[1]) == R.HELD for r in d.ref.ring[:min(appends, 4)])
    if with_acc and appends == 6:
        assert counts.tolist() == [4, 1, 1, 1] and out[2, 3] == 2 and out[3, 3] == 2      # rows 2..5: held, applied, dropped(-inf), applied


def test_held_only_window(cuda):
    rng = np.random.RandomState(5)
    d = _Dev(4, 12, cuda, False)
    d.append(*_row(rng, 12, 0, R.APPLIED, False))
    for k in range(1, 4):
        d.append(*_row(rng, 12, k, R.HELD, False))
    out, counts = d.check_window(3)
    assert counts.tolist() == [3, 3, 0, 0] and not out.any()
    out, counts = d.check_window(4)
    assert counts.tolist() == [4, 3, 0, 0] and out[2, 3] == 1


def test_long_window_over_several_chunks(cuda):
    """More rows than the window kernel stages at once (256), in a wrapped ring: the float64 order still holds."""
    rng = np.random.RandomState(6)
    cap, n = 600, 700
    d = _Dev(cap, 1, cuda, False)
    vals = (rng.uniform(-1, 1, n) * 10.0 ** rng.randint(-3, 8, n)).astype(np.float32)
    st = _row(rng, 1, 0, R.APPLIED, False)[2]
    # the device ring is written in one copy (700 single appends would test nothing more), the cursor set to match
    for k in range(n):
        d.ref.append([vals[k]], vals[k], st)
    d.ring.copy_(torch.from_numpy(d.ref.ring.view(np.int32)))
    d.cursor.fill_(n)
    for last in (255, 256, 257, 600, 4096):
        d.check_window(last)


def test_captured_append_follows_the_cursor(cuda):
    d = _Dev(4, 12, cuda, True)
    rng = np.random.RandomState(7)
    terms, total, st, acc = _row(rng, 12, 0, R.APPLIED, True)
    d.terms.copy_(torch.from_numpy(terms)); d.total.fill_(float(total)); d.state.copy_(torch.from_numpy(st)); d.acc.copy_(torch.from_numpy(acc))
    ptrs = [d.terms[i] for i in range(12)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        nv.step_log_append(ptrs, d.total, d.state, d.acc, d.ring, d.cursor)       # warm-up launch: row 0
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        nv.step_log_append(ptrs, d.total, d.state, d.acc, d.ring, d.cursor)
    torch.cuda.synchronize()
    assert int(d.cursor.item()) == 1                          # the capture itself ran nothing
    d.ring.zero_(); d.cursor.zero_()
    for k in range(5):
        d.total.fill_(float(k))                               # the static inputs change between replays
        with _no_host_sync():
            g.replay()
        d.ref.append(terms, float(k), st, acc)
    d.check_ring()
    ring = d.ring.cpu().numpy()
    assert int(d.cursor.item()) == 5 and sorted(ring[:, 0].tolist()) == [1, 2, 3, 4]
    assert ring[0, 0] == 4 and ring[0].view(np.float32)[2] == 4.0             # row 4 wrapped into slot 0
    d.check_window(50)


def test_append_and_window_launch_without_host_sync(cuda):
    d = _Dev(4, 36, cuda, False)
    rng = np.random.RandomState(8)
    terms, total, st, _ = _row(rng, 36, 0, R.APPLIED, False)
    d.terms.copy_(torch.from_numpy(terms)); d.total.fill_(float(total)); d.state.copy_(torch.from_numpy(st))
    ptrs = [d.terms[i] for i in range(36)]
    with _no_host_sync():
        nv.step_log_append(ptrs, d.total, d.state, None, d.ring, d.cursor)
        nv.step_log_window(d.ring, d.cursor, 50, d.out, d.counts)
    d.ref.append(terms, total, st)
    d.check_ring()


def test_refusals_write_nothing(cuda):
    d = _Dev(4, 2, cuda, False)
    d.ring.fill_(-3); d.cursor.fill_(2)
    lib = nv.lib()
    p = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731
    big = (C.c_void_p * 65)(*[d.terms.data_ptr()] * 65)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ARG = -1
    assert lib.u3d_step_log_append(big, 65, p(d.total), p(d.state), None, p(d.ring), p(d.cursor), 4, stream) == ARG
    assert lib.u3d_step_log_append(big, 2, p(d.total), p(d.state), None, p(d.ring), p(d.cursor), 0, stream) == ARG
    assert lib.u3d_step_log_append(big, 2, None, p(d.state), None, p(d.ring), p(d.cursor), 4, stream) == ARG
    assert lib.u3d_step_log_append(big, 2, p(d.total), p(d.state), None, None, p(d.cursor), 4, stream) == ARG
    big[1] = None
    assert lib.u3d_step_log_append(big, 2, p(d.total), p(d.state), None, p(d.ring), p(d.cursor), 4, stream) == ARG
    assert lib.u3d_step_log_window(p(d.ring), p(d.cursor), 0, 2, 4, p(d.out), p(d.counts), stream) == ARG
    assert lib.u3d_step_log_window(p(d.ring), p(d.cursor), 4, 65, 4, p(d.out), p(d.counts), stream) == ARG
    assert lib.u3d_step_log_window(p(d.ring), None, 4, 2, 4, p(d.out), p(d.counts), stream) == ARG
    torch.cuda.synchronize()
    assert int(d.cursor.item()) == 2 and bool((d.ring == -3).all()) and bool((d.out == -7).all()) and bool((d.counts == -7).all())
    with pytest.raises(ValueError):
        StepLog(capacity=0, device=cuda)


def test_steplog_object_rows_window_and_state(cuda):
    log = StepLog(capacity=4, device=cuda)
    names = ["loss_cls", "loss_bbox", "d0.loss_cls"]
    ref = R.StepLogRef(4, 3)
    rng = np.random.RandomState(9)
    state = torch.zeros(16, device=cuda)
    for k in range(6):
        terms, total, st, _ = _row(rng, 3, k, R.HELD if k == 4 else R.APPLIED, False)
        state.copy_(torch.from_numpy(st))
        log.append({n: torch.tensor(float(v), device=cuda) for n, v in zip(names, terms)}, torch.tensor(float(total), device=cuda), state)
        ref.append(terms, total, st)
    assert len(log) == 6 and log.columns[8:] == names
    rows = log.rows(2, 4)
    assert rows[:, 0].tolist() == [2, 3, 4, 5] and rows[:, 1].tolist() == [1, 1, 3, 1]
    assert np.array_equal(rows.view(np.uint32), np.stack([ref.ring[k % 4] for k in range(2, 6)]))
    with pytest.raises(IndexError):
        log.rows(1, 2)                                        # row 1 has left the ring
    w = log.window(3)
    want, counts = ref.window(3)
    assert (w["steps"], w["held"], w["dropped"], w["nonfinite"], w["used"]) == (3, 1, 0, 0, 2)
    assert w["loss"] == float(want[2, 0]) and w["grad_norm"] == float(want[3, 0]) and w["lr"] == float(want[5, 0])
    assert w["d0.loss_cls"] == float(want[10, 0])
    with pytest.raises(ValueError):
        log.append({"other": state[0]}, state[1], state)       # the columns were fixed by the first step
    other = StepLog(capacity=4, device=cuda)
    other.load_state_dict(log.state_dict())
    assert len(other) == 6 and other.names == names and np.array_equal(other.rows(2, 4), rows) and other.window(3) == w
