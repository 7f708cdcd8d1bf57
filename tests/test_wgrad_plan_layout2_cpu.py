"""CPU: u3d_igemm_wgrad_plan for out_layout 2 (the weight gradient with the operands exchanged, summed over a sparse level's active
rows).  The layout only chooses the reduction: wherever the tiled families serve a shape, the plan is the one of out_layout 1;
the conv-in and narrow families, more than 27 offsets and unknown layouts are not served."""
import ctypes

import pytest

from uni3detr_amd import native as nv


@pytest.mark.parametrize("n,cin,cout,kvol", [(60000, 128, 256, 9), (192000, 256, 256, 9), (430, 128, 128, 9), (54000, 512, 256, 9),
                                             (0, 128, 128, 9), (7200, 256, 256, 1), (5000, 48, 80, 27), (5000, 32, 32, 9)])
def test_layout2_plan_is_the_layout1_plan(n, cin, cout, kvol):
    p1, p2 = nv.igemm_wgrad_plan(n, cin, cout, kvol, True, out_oik=True), nv.igemm_wgrad_plan(n, cin, cout, kvol, True, out_layout=2)
    assert p1 is not None and p2 == p1
    assert p2[3] == p2[2] * kvol * cin * cout * 4


@pytest.mark.parametrize("n,cin,cout,kvol", [(5000, 16, 16, 27), (5000, 32, 64, 27), (5000, 8, 16, 27), (5000, 64, 64, 28), (5000, 24, 64, 9)])
def test_layout2_is_not_served_off_the_tiled_families(n, cin, cout, kvol):
    assert nv.igemm_wgrad_plan(n, cin, cout, kvol, True, out_layout=2) is None


def test_unknown_layout_is_refused():
    k, t, ns, ws = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0)
    rc = nv.lib().u3d_igemm_wgrad_plan(1000, 64, 64, 9, 1, 3, ctypes.byref(k), ctypes.byref(t), ctypes.byref(ns), ctypes.byref(ws))
    assert rc == nv.U3D_ERR_UNSUPPORTED
