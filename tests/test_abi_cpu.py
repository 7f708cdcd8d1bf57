"""uni3detr_amd/abi.py: the reader of include/u3d_hip.h on a small header with literal expected output, each of its refusals, the real
header against the built library and the bindings native.lib() sets, and literal pins of signatures, constants and struct sizes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from uni3detr_amd import abi
from uni3detr_amd import native as nv

P, I, L, F = C.c_void_p, C.c_int32, C.c_int64, C.c_float

SMALL = """
/* a block comment with a declaration: int32_t u3d_fake(int32_t x);
 * over two lines */
#ifndef SMALL_H_
#define SMALL_H_
#include <stdint.h>
#define U3D_CAP 2048    /* a trailing comment */
#define U3D_HEX 0x10
#define U3D_TWICE(x) (2 * (x))
typedef struct ihipStream_t* u3d_stream;
enum { U3D_OK = 0, U3D_ERR_ARG = -1, U3D_ERR_OTHER = -7 };
enum {
  U3D_S_A, U3D_S_B,   // int32_t u3d_fake(int32_t x);
  U3D_S_C,
  U3D_S_COUNT
};
enum { U3D_T_X = 5, U3D_T_Y };
typedef struct u3d_tagged {
  void* words;
  int32_t batch, dz, dy, dx;
  float p_attn, p_drop;
  const void* w[U3D_S_COUNT];
  int64_t off[2], total;
} u3d_tagged;
typedef struct {
  const float* mean; const float* invstd;
  int32_t relu;
} u3d_anon;
int32_t u3d_version(void);
const char* u3d_strerror(int32_t code);
int64_t u3d_three_lines(const u3d_tagged* g, const int32_t* coors,
                        int32_t n, const float v[3],
                        float eps, int64_t bytes, u3d_stream s);
int32_t u3d_pointers(void** event, const void* const* srcs, const u3d_anon* bn);
float u3d_ratio(const int32_t n);
#endif
"""


def test_reader_on_a_small_header():
    a = abi.parse(SMALL)
    assert a.prototypes == {
        "u3d_version": (I, []),
        "u3d_strerror": (C.c_char_p, [I]),
        "u3d_three_lines": (L, [P, P, I, P, F, L, P]),
        "u3d_pointers": (I, [P, P, P]),
        "u3d_ratio": (F, [I]),
    }
    assert a.constants == {"U3D_CAP": 2048, "U3D_HEX": 16, "U3D_OK": 0, "U3D_ERR_ARG": -1, "U3D_ERR_OTHER": -7, "U3D_S_A": 0, "U3D_S_B": 1,
                           "U3D_S_C": 2, "U3D_S_COUNT": 3, "U3D_T_X": 5, "U3D_T_Y": 6}
    assert a.structs == {
        "u3d_tagged": [("words", "pointer", None), ("batch", "int32_t", None), ("dz", "int32_t", None), ("dy", "int32_t", None),
                       ("dx", "int32_t", None), ("p_attn", "float", None), ("p_drop", "float", None), ("w", "pointer", 3),
                       ("off", "int64_t", 2), ("total", "int64_t", None)],
        "u3d_anon": [("mean", "pointer", None), ("invstd", "pointer", None), ("relu", "int32_t", None)],
    }
    s = abi.structure(a.structs["u3d_tagged"], "Tagged")
    assert s.__name__ == "Tagged" and issubclass(s, C.Structure)
    assert s._fields_ == [("words", P), ("batch", I), ("dz", I), ("dy", I), ("dx", I), ("p_attn", F), ("p_drop", F), ("w", P * 3),
                          ("off", L * 2), ("total", L)]
    assert C.sizeof(s) == 8 + 16 + 8 + 24 + 16 + 8
    d = abi.numpy_dtype(a.structs["u3d_tagged"])
    assert d.itemsize == C.sizeof(s) and d.names == tuple(n for n, _ in s._fields_)
    assert [d.fields[n][1] for n in d.names] == [getattr(s, n).offset for n in d.names] and d["w"].shape == (3,)
    assert abi.numpy_dtype(a.structs["u3d_anon"]).itemsize == C.sizeof(abi.structure(a.structs["u3d_anon"], "Anon")) == 24    # tail padding


@pytest.mark.parametrize("text, match", [
    ("int32_t u3d_f(double x);", "by value"),                                                 # an unknown by-value type
    ("int32_t u3d_f(int32_t a, uint8_t flag);", "by value"),
    ("double u3d_f(int32_t a);", "return type"),
    ("typedef struct { double x; } u3d_s;", "field declaration"),                             # an unknown field type
    ("typedef struct { float* a, b; } u3d_s;", "field declaration"),                          # `float* a, b` makes b a float in C: refused
    ("typedef struct { int32_t a[U3D_NOWHERE]; } u3d_s;", "array length"),                    # an unresolvable array length
    ("typedef struct { int32_t a[2][2]; } u3d_s;", "declarator"),
    ("int32_t u3d_f(int32_t a);\nint32_t u3d_f(int32_t a);", "declared twice"),               # a duplicate name
    ("int32_t u3d_f(int32_t a);\nint32_t u3d_g(int32_t (*cb)(int32_t));", "2 occurrences"),   # a prototype the pattern misses
    ("int32_t u3d_f(int32_t a) { return a; }", "1 occurrences"),
    ("enum { U3D_A = 1 << 3 };", "enumerator"),
])
def test_reader_refuses(text, match):
    with pytest.raises(abi.AbiError, match=match):
        abi.parse(text)


def test_missing_header_names_the_path(monkeypatch):
    gone = os.path.join(os.path.dirname(abi.HEADER), "no_such_header.h")
    monkeypatch.setattr(abi, "HEADER", gone)
    abi.load.cache_clear()
    try:
        with pytest.raises(FileNotFoundError, match="no_such_header.h"):
            abi.load()
    finally:
        abi.load.cache_clear()


def test_abi_needs_neither_torch_nor_native():
    src = open(abi.__file__).read()
    assert not re.search(r"^\s*(import|from)\s+(torch|\.native|uni3detr_amd)", src, re.M)
    assert os.path.samefile(abi.HEADER, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "u3d_hip.h"))


def test_real_header_is_read_whole_and_bound_as_read():
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(abi.HEADER).read(), flags=re.S)
    protos = abi.load().prototypes
    assert len(protos) == len(re.findall(r"u3d_[a-z0-9_]+\(", text)) > 100
    raw = C.CDLL(nv.LIB_PATH)
    for name in protos:
        assert hasattr(raw, name), f"{name} declared in include/u3d_hip.h but not exported"
    lib = nv.lib()
    for name, (res, args) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert nv.exported_symbols() == sorted(protos)


def test_signature_pins():
    p = abi.load().prototypes
    assert p["u3d_det_tail"] == (I, [P] * 3 + [I] * 5 + [P, F, I, F, P, I] + [P] * 6 + [L, P]) and len(p["u3d_det_tail"][1]) == 22
    assert p["u3d_det_tail_workspace"] == (L, [I] * 5)
    # u3d_det_tail_pp = u3d_det_tail's list with soft_sigma, soft_prune after num_thr; the workspace query gains the mode
    old, new = p["u3d_det_tail"][1], p["u3d_det_tail_pp"][1]
    assert new == old[:14] + [F, F] + old[14:] and p["u3d_det_tail_pp"][0] is I
    assert p["u3d_det_tail_pp_workspace"] == (L, p["u3d_det_tail_workspace"][1] + [I])
    assert len(p["u3d_adamw_step_accum"][1]) == 14 and len(p["u3d_adamw_set_accum"][1]) == 4
    assert [(p[n][0], len(p[n][1])) for n in ("u3d_gtdb_count", "u3d_gtdb_scan", "u3d_gtdb_crop")] == [(I, 15), (I, 7), (I, 18)]
    assert p["u3d_version"] == (I, []) and p["u3d_strerror"] == (C.c_char_p, [I])


def test_constant_pins():
    k = abi.load().constants
    assert [k["U3D_DET_TAIL_" + n] for n in ("NONE", "NMS", "DECODE", "SOFT_NMS", "MERGE")] == [0, 1, 2, 3, 4]
    assert (nv.DET_TAIL_NONE, nv.DET_TAIL_NMS, nv.DET_TAIL_DECODE, nv.DET_TAIL_SOFT_NMS, nv.DET_TAIL_MERGE) == (0, 1, 2, 3, 4)
    assert k["U3D_DET_TAIL_MAX_K"] == nv.DET_TAIL_MAX_K == 8192
    assert (k["U3D_OK"], k["U3D_ERR_ARG"], nv.U3D_ERR_UNSUPPORTED, k["U3D_ERR_LAUNCH"], k["U3D_ERR_WORKSPACE"]) == (0, -1, -2, -3, -4)
    assert (nv.F32, nv.BF16, nv.DT_F32, nv.DT_BF16) == (0, 1, 0, 1)
    assert (nv.DL_RPH0, nv.DL_INQK, nv.DL_IOU2, nv.DL_NLIN, nv.DLN_1, nv.DLN_C2, nv.DL_NLN) == (0, 6, 21, 22, 0, 6, 7)
    assert len(nv.DS_NAMES) == 33 and nv.DS_NAMES[0] == "SINE" and nv.DS_NAMES[-1] == "AMASK" and nv.DS_NAMES.index("LSE") == 11
    assert len(nv.DG_NAMES) == 29 and nv.DG_NAMES[0] == "CLSO" and nv.DG_NAMES[-1] == "SINE" and nv.DG_NAMES.index("LNP") == 25
    assert (nv.AUG_NPARAM, nv.TTA_LDS_CAP, nv.SWEEPS_CHUNK, nv.SWEEPS_NPARAM) == (9, 2048, 256, 13)
    assert (nv.SWEEP_SEG_KEY, nv.SWEEP_SEG_SWEEP, nv.SWEEP_SEG_PAD) == (0, 1, 2)


def test_struct_size_pins():
    """The sizes of the hand-written classes these layouts replaced: the derived layouts are the ones the kernels read."""
    s = abi.load().structs
    assert sorted(s) == sorted(["u3d_bitgrid", "u3d_declayer_params", "u3d_declayer_dims", "u3d_wpack_desc", "U3dSplitRowsJobs",
                                "u3d_permute_desc", "u3d_fwd_plan_info", "u3d_bn_fold_job", "u3d_bn_fold_fp8_job", "u3d_split3_job"])
    for cls, size in ((nv.BitGridStruct, 40), (nv.DecLayerParams, 680), (nv.DecLayerDims, 68), (nv.WPackDesc, 48),
                      (nv._SplitRowsJobs, 1032), (nv.FwdPlanInfo, 28), (nv.BnFoldJob, 104), (nv.BnFoldFp8Job, 112),
                      (nv.Split3Set._Job, 56)):
        assert C.sizeof(cls) == size and issubclass(cls, C.Structure), cls
    assert np.dtype(nv.PERMUTE_DESC_DTYPE).itemsize == 56
    assert [n for n, _ in nv.BitGridStruct._fields_] == ["words", "prefix", "batch", "dz", "dy", "dx", "layout", "row_capacity"]
    assert [n for n, _ in nv.BnFoldJob._fields_] == ["w", "gamma", "beta", "mean", "var", "w_folded", "shift", "sk", "sa", "sb", "eps",
                                                     "kvol", "cout", "cin", "scale_only", "first_block"]
