"""The step log without a device: the numpy restatement (tests/step_log_ref.py) on hand-checked cases, the three C-ABI entries in the
header-derived binding, the header's constant against the Python one, and the entries' refusals (answered before any launch)."""
import ctypes as C

import numpy as np

import step_log_ref as R
from uni3detr_amd import abi
from uni3detr_amd import native as nv
from uni3detr_amd import step_log as SL

P, I, L = C.c_void_p, C.c_int32, C.c_int64


def _state(held=False, norm=2.0, coef=0.5, lr=1e-3, beta1=0.9):
    st = np.zeros(16, np.float32)
    st[1], st[4], st[5], st[6], st[11] = coef, norm, lr, beta1, 1.0 if held else 0.0
    return st


def test_abi_has_the_three_entries():
    p = abi.load().prototypes
    assert p["u3d_step_log_bytes"] == (L, [L, I])
    assert p["u3d_step_log_append"] == (I, [P, I, P, P, P, P, P, L, P])
    assert p["u3d_step_log_window"] == (I, [P, P, L, I, L, P, P, P])
    lib = nv.lib()
    for name in ("u3d_step_log_bytes", "u3d_step_log_append", "u3d_step_log_window"):
        assert name in nv.exported_symbols() and getattr(lib, name).restype is p[name][0]


def test_constants_agree():
    k = abi.load().constants
    assert k["U3D_STEP_LOG_FIXED"] == SL.STEP_LOG_FIXED == R.FIXED == 8 == len(SL.FIXED_NAMES)
    assert k["U3D_STEP_LOG_MAX_TERMS"] == SL.MAX_TERMS == 64
    assert (SL.ACCUMULATED, SL.APPLIED, SL.DROPPED, SL.HELD) == (R.ACCUMULATED, R.APPLIED, R.DROPPED, R.HELD) == (0, 1, 2, 3)
    assert nv.step_log_bytes(4096, 12) == 4096 * 20 * 4 and nv.step_log_bytes(1, 0) == 32
    assert nv.step_log_bytes(0, 12) == 0 and nv.step_log_bytes(4, 65) == 0 and nv.step_log_bytes(4, -1) == 0


def test_refusals_before_any_launch():
    buf = (C.c_char * 1024)()
    h = [C.c_void_p(C.addressof(buf) + 64 * i) for i in range(8)]
    lib, ARG = nv.lib(), abi.load().constants["U3D_ERR_ARG"]
    terms = (C.c_void_p * 65)(*[h[0].value] * 65)
    assert lib.u3d_step_log_append(terms, 65, h[1], h[2], None, h[3], h[4], 4, None) == ARG
    assert lib.u3d_step_log_append(terms, 2, h[1], h[2], None, h[3], h[4], 0, None) == ARG
    assert lib.u3d_step_log_append(None, 2, h[1], h[2], None, h[3], h[4], 4, None) == ARG
    assert lib.u3d_step_log_append(terms, 2, None, h[2], None, h[3], h[4], 4, None) == ARG
    assert lib.u3d_step_log_append(terms, 2, h[1], None, None, h[3], h[4], 4, None) == ARG
    assert lib.u3d_step_log_append(terms, 2, h[1], h[2], None, None, h[4], 4, None) == ARG
    assert lib.u3d_step_log_append(terms, 2, h[1], h[2], None, h[3], None, 4, None) == ARG
    terms[1] = None
    assert lib.u3d_step_log_append(terms, 2, h[1], h[2], None, h[3], h[4], 4, None) == ARG
    assert lib.u3d_step_log_window(h[3], h[4], 4, 65, 2, h[5], h[6], None) == ARG
    assert lib.u3d_step_log_window(h[3], h[4], 0, 2, 2, h[5], h[6], None) == ARG
    assert lib.u3d_step_log_window(h[3], h[4], 4, 2, -1, h[5], h[6], None) == ARG
    assert lib.u3d_step_log_window(None, h[4], 4, 2, 2, h[5], h[6], None) == ARG
    assert lib.u3d_step_log_window(h[3], h[4], 4, 2, 2, None, h[6], None) == ARG
    assert bytes(buf) == bytes(1024)


def test_ref_ring_and_row_layout():
    r = R.StepLogRef(4, 2)
    for k in range(6):
        r.append([k + 0.25, k + 0.5], float(k), _state(held=(k == 4), norm=10.0 + k, lr=0.001 * (k + 1)))
    assert r.cursor == 6
    # rows 2, 3 stay in slots 2, 3; rows 4, 5 wrapped into slots 0, 1
    assert r.ring[:, 0].view(np.int32).tolist() == [4, 5, 2, 3]
    assert r.ring[:, 1].tolist() == [R.HELD, R.APPLIED, R.APPLIED, R.APPLIED]
    f = r.ring.view(np.float32)
    assert f[1, 2] == 5.0 and f[1, 3] == 15.0 and f[1, 4] == 0.5 and f[1, 5] == np.float32(0.006) and f[1, 6] == np.float32(0.9)
    assert r.ring[1, 7] == 0 and f[1, 8:].tolist() == [5.25, 5.5]


def test_ref_acc_state_outcomes_and_window_rules():
    r = R.StepLogRef(8, 1)
    acc = np.zeros(8, np.float32)
    totals = [1.0, 2.0, np.nan, 4.0, 5.0, np.inf]
    outcomes = [R.ACCUMULATED, R.APPLIED, R.APPLIED, R.HELD, R.DROPPED, R.APPLIED]
    for t, o in zip(totals, outcomes):
        acc[5], acc[6] = o, 3.0 if o == R.APPLIED else 7.0
        r.append([2 * t], t, _state(norm=99.0, coef=0.25), acc)
    out, counts = r.window(50)
    assert counts.tolist() == [6, 1, 1, 2]                   # the held row's total is not looked at
    assert out[2].tolist() == [float(np.float32(8 / 3)), 1.0, 5.0, 3.0]
    assert out[3].tolist() == [3.0, 3.0, 3.0, 3.0]           # applied rows only (their norm is acc_state[6]); NaN totals do not unuse a row
    assert out[4].tolist() == [0.25, 0.25, 0.25, 3.0]
    assert out[8].tolist() == [float(np.float32(16 / 3)), 2.0, 10.0, 3.0]
    assert not out[:2].any()
    out, counts = r.window(2)                                # rows 4, 5: dropped, applied with an Inf total
    assert counts.tolist() == [2, 0, 1, 1] and out[2].tolist() == [5.0, 5.0, 5.0, 1.0] and out[3, 3] == 1.0


def test_ref_held_only_window_and_empty_log():
    r = R.StepLogRef(4, 3)
    out, counts = r.window(10)
    assert not out.any() and not counts.any()
    for k in range(3):
        r.append([1.0, 2.0, 3.0], 6.0, _state(held=True))
    out, counts = r.window(10)
    assert counts.tolist() == [3, 3, 0, 0] and not out.any()
    out, counts = r.window(0)
    assert counts.tolist() == [0, 0, 0, 0]


def test_ref_mean_is_one_rounding_of_a_float64_sum():
    r = R.StepLogRef(16, 1)
    vals = np.float32([1e8, 1.0, -1e8, 1.0, 3.0, 1e-3])
    for v in vals:
        r.append([v], v, _state())
    out, _ = r.window(16)
    assert out[2, 0] == np.float32(np.sum(vals.astype(np.float64)) / 6) != np.float32(np.sum(vals) / np.float32(6))
