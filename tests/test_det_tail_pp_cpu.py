"""The soft-NMS / box-merging modes of the batched inference tail without a GPU: the two entry points are part of the build (their
signatures, and how they extend u3d_det_tail's, are pinned in tests/test_abi_cpu.py), and the mode constants."""
from uni3detr_amd import native as nv


def test_pp_entry_points_declared_and_bound():
    for name in ("u3d_det_tail_pp_workspace", "u3d_det_tail_pp"):
        assert name in nv.exported_symbols()


def test_mode_constants_agree():
    assert (nv.DET_TAIL_SOFT_NMS, nv.DET_TAIL_MERGE) == (3, 4)
    assert (nv.DET_TAIL_NONE, nv.DET_TAIL_NMS, nv.DET_TAIL_DECODE) == (0, 1, 2)
