"""The soft-NMS / box-merging modes of the batched inference tail without a GPU: the two entry points declared in include/u3d_hip.h
as native._SIGS binds them, and the mode constants on both sides."""
import os
import re

from uni3detr_amd import native as nv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pp_entry_points_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "u3d_hip.h")).read()
    ctype = {"int32_t": nv.C.c_int32, "int64_t": nv.C.c_int64, "float": nv.C.c_float}
    for name, restype in (("u3d_det_tail_pp_workspace", "int64_t"), ("u3d_det_tail_pp", "int32_t")):
        m = re.search(restype + r"\s+" + name + r"\(([^;]*)\);", hdr)
        assert m, name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        res, args = nv._SIGS[name]
        assert res is ctype[restype] and len(args) == len(params), (name, len(args), len(params))
        for p, a in zip(params, args):
            base = p.rsplit(" ", 1)[0].replace("const ", "").strip()
            want = nv.C.c_void_p if ("*" in p or base == "u3d_stream") else ctype[base]
            assert a is want, (name, p)
        assert name in nv.exported_symbols()


def test_pp_takes_every_argument_of_det_tail_plus_sigma_and_prune():
    """u3d_det_tail_pp = u3d_det_tail's list with soft_sigma, soft_prune after num_thr; the workspace query gains the mode."""
    _, old = nv._SIGS["u3d_det_tail"]
    _, new = nv._SIGS["u3d_det_tail_pp"]
    assert list(new) == list(old[:14]) + [nv.C.c_float, nv.C.c_float] + list(old[14:])
    assert list(nv._SIGS["u3d_det_tail_pp_workspace"][1]) == list(nv._SIGS["u3d_det_tail_workspace"][1]) + [nv.C.c_int32]


def test_mode_constants_agree():
    hdr = open(os.path.join(ROOT, "include", "u3d_hip.h")).read()
    for k in ("U3D_DET_TAIL_SOFT_NMS 3", "U3D_DET_TAIL_MERGE 4"):
        assert re.search(r"#define\s+" + k + r"\b", hdr), k
    assert (nv.DET_TAIL_SOFT_NMS, nv.DET_TAIL_MERGE) == (3, 4)
    assert (nv.DET_TAIL_NONE, nv.DET_TAIL_NMS, nv.DET_TAIL_DECODE) == (0, 1, 2)
