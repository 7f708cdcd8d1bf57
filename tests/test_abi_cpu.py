"""uni3detr_amd/abi.py: the reader of include/u3d_hip.h on a small header with literal expected output, each of its refusals, the real
header against the built library and the bindings native.lib() sets, literal pins of signatures, constants and struct sizes - and the
one-entry-per-operation rule: every export is named by the package, the retired variant / wrapper names are gone, and the merged
entries answer their argument and shape checks before any launch (no GPU involved)."""
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
                                "u3d_permute_desc", "u3d_fwd_plan_info", "u3d_bn_fold_job", "u3d_bn_fold_fp8_job", "u3d_split3_job",
                                "u3d_halo_tables"])
    for cls, size in ((nv.BitGridStruct, 40), (nv.DecLayerParams, 680), (nv.DecLayerDims, 68), (nv.WPackDesc, 48),
                      (nv._SplitRowsJobs, 1032), (nv.FwdPlanInfo, 28), (nv.BnFoldJob, 104), (nv.BnFoldFp8Job, 112),
                      (nv.Split3Set._Job, 56), (nv.HaloTables, 40)):
        assert C.sizeof(cls) == size and issubclass(cls, C.Structure), cls
    assert np.dtype(nv.PERMUTE_DESC_DTYPE).itemsize == 56
    assert [n for n, _ in nv.BitGridStruct._fields_] == ["words", "prefix", "batch", "dz", "dy", "dx", "layout", "row_capacity"]
    assert [n for n, _ in nv.HaloTables._fields_] == ["tile_rows", "loc", "tile_cnt", "n_dev", "n_cap", "kvol"]
    assert [n for n, _ in nv.BnFoldJob._fields_] == ["w", "gamma", "beta", "mean", "var", "w_folded", "shift", "sk", "sa", "sb", "eps",
                                                     "kvol", "cout", "cin", "scale_only", "first_block"]


# The suffix variants, wrapper exports and orphans that one entry per operation replaced (HISTORY.md).  The plain names of the
# renamed long forms (u3d_mha_fwd, u3d_decoder_layer_slots, ...) live on with the long forms' signatures: test_merged_signatures.
RETIRED = ("u3d_subm_halo_conv64_bf16", "u3d_subm_halo_conv128_bf16", "u3d_subm_halo_conv64_affine_bf16",
           "u3d_subm_halo_conv128_affine_bf16", "u3d_subm_halo_wpack128", "u3d_subm_halo_wpack128_batched",
           "u3d_bn_apply_planes", "u3d_bn_bwd_apply_planes", "u3d_mha_fwd_dt", "u3d_mha_bwd_dt", "u3d_decoder_layer_fwd_nw",
           "u3d_decoder_layer_bwd_nw", "u3d_decoder_layer_slots_dt", "u3d_decoder_layer_blocks_dt", "u3d_wpack_bf16",
           "u3d_adamw_step_state", "u3d_tap_gather_sum_add", "u3d_bitgrid_nwords", "u3d_nusc_match_lds", "u3d_kitti_compact",
           "u3d_nusc_compact")
OK, ARG, UNSUPPORTED = 0, -1, -2


def test_every_export_is_named_by_the_package():
    pkg = os.path.dirname(os.path.abspath(nv.__file__))
    text = "\n".join(open(os.path.join(d, f)).read() for d, _, fs in os.walk(pkg) for f in fs if f.endswith(".py"))
    words = set(re.findall(r"\bu3d_[a-z0-9_]+\b", text))
    assert not [n for n in nv.exported_symbols() if n not in words]


def test_retired_names_are_gone():
    declared = set(re.findall(r"\bu3d_[a-z0-9_]+\b", open(abi.HEADER).read()))
    raw = C.CDLL(nv.LIB_PATH)
    for name in RETIRED:
        assert name not in declared and name not in nv.exported_symbols() and not hasattr(raw, name), name


def test_merged_signatures():
    p = abi.load().prototypes
    assert p["u3d_subm_halo_conv_bf16"] == (I, [P, P, P, I, I, P, P, P, P, I, I, P])
    assert p["u3d_subm_halo_wpack"] == (I, [P, P, I, I, P]) and p["u3d_subm_halo_wpack_batched"] == (I, [P, P, I, I, I, P])
    assert p["u3d_subm_halo_wgrad64_bf16"] == (I, [P, P, P, P, P, L, I, P])
    assert p["u3d_bn_apply"] == (I, [P] * 6 + [I, P, P, P, I, I, I, P, P, P])                   # planes after y
    assert p["u3d_bn_bwd_apply"] == (I, [P] * 8 + [I, P, P, P, P, I, I, I, P, P])               # planes after dres
    assert p["u3d_mha_fwd"][1][-2:] == [I, P] and p["u3d_mha_bwd"][1][-2:] == [I, P]            # dtype, stream
    assert p["u3d_decoder_layer_fwd"][1][-3:] == [L, I, P] and p["u3d_decoder_layer_bwd"][1][-3:] == [L, I, P]      # .., row_waves, stream
    assert p["u3d_decoder_layer_slots"] == (I, [I, I, I, I, P, P]) and p["u3d_decoder_layer_blocks"] == (I, [I, I])
    assert p["u3d_tap_gather_sum"] == (I, [P, P, I, P, I, I, I, I, P, P, P])                    # addend before out


class _Host:
    """64-byte-aligned addresses inside one host buffer, standing in for device pointers the calls never dereference."""

    def __init__(self, n=16):
        self.buf = (C.c_char * (64 * (n + 1)))()
        self.base = (C.addressof(self.buf) + 63) & ~63

    def __getitem__(self, i):
        return C.c_void_p(self.base + 64 * i)


def _halo_tables(h, n_cap=256, kvol=27):
    return nv.HaloTables(h[0].value, h[1].value, h[2].value, h[3].value, n_cap, kvol)


@pytest.mark.parametrize("c, kvol, krev, stats, shift, relu, want", [
    (96, 27, 0, False, False, 0, UNSUPPORTED),
    (64, 9, 0, False, False, 0, UNSUPPORTED),
    (64, 27, 0, True, True, 0, ARG),            # the affine epilogue reduces no statistics
    (64, 27, 1, False, True, 0, ARG),           # ... and is forward only
    (128, 9, 1, False, True, 1, ARG),
    (64, 27, 0, False, False, 1, ARG),          # a ReLU needs the affine epilogue
    (128, 28, 0, False, False, 0, ARG),         # more offsets than loc holds
    (96, 27, 1, False, True, 0, ARG),           # argument checks come before shape checks
])
def test_halo_conv_return_codes(c, kvol, krev, stats, shift, relu, want):
    h = _Host()
    t = _halo_tables(h, kvol=kvol)
    rc = nv.lib().u3d_subm_halo_conv_bf16(h[4], h[5], C.byref(t), c, krev, None, h[6], h[7] if stats else None, h[8] if shift else None,
                                          relu, 0, None)
    assert rc == want


def test_halo_null_and_wpack_return_codes():
    h = _Host()
    lib = nv.lib()
    assert lib.u3d_subm_halo_conv_bf16(h[4], h[5], None, 64, 0, None, h[6], None, None, 0, 0, None) == ARG
    t = _halo_tables(h)
    t.loc = None
    assert lib.u3d_subm_halo_conv_bf16(h[4], h[5], C.byref(t), 64, 0, None, h[6], None, None, 0, 0, None) == ARG
    assert lib.u3d_subm_halo_wpack(h[0], h[1], 64, 9, None) == UNSUPPORTED
    assert lib.u3d_subm_halo_wpack(h[0], h[1], 32, 27, None) == UNSUPPORTED
    assert lib.u3d_subm_halo_wpack(h[0], None, 64, 27, None) == ARG
    assert lib.u3d_subm_halo_wpack_batched(h[0], h[1], 2, 64, 9, None) == UNSUPPORTED
    assert lib.u3d_subm_halo_wpack_batched(h[0], h[1], 0, 128, 9, None) == OK       # nothing to pack: no launch
    assert lib.u3d_subm_halo_wpack_batched(h[0], h[1], -1, 128, 9, None) == ARG
    t9 = _halo_tables(h, kvol=9)
    assert lib.u3d_subm_halo_wgrad64_bf16(h[4], h[5], C.byref(t9), h[6], h[7], 1 << 40, 0, None) == UNSUPPORTED


@pytest.mark.parametrize("planes", [False, True])
def test_bn_planes_return_codes(planes):
    h = _Host()
    lib = nv.lib()
    pl = h[9] if planes else None

    def fwd(n_cap, c, dtype):       # x mean invstd gamma beta residual relu y planes n_dev n_cap c dtype row_map post_add stream
        return lib.u3d_bn_apply(h[0], h[1], h[2], h[3], h[4], None, 1, h[5], pl, h[6], n_cap, c, dtype, None, None, None)

    def bwd(n_cap, c, dtype):       # dy y x mean invstd gamma beta sums relu dx dres planes n_dev n_cap c dtype row_map stream
        return lib.u3d_bn_bwd_apply(h[0], h[7], h[8], h[1], h[2], h[3], h[4], h[10], 1, h[5], None, pl, h[6], n_cap, c, dtype, None, None)

    for call in (fwd, bwd):
        assert call(0, 64, nv.F32) == OK                          # no rows: nothing launched
        if planes:
            assert call(0, 64, nv.BF16) == UNSUPPORTED            # the planes come from f32 rows only
            assert call(0, 24, nv.F32) == UNSUPPORTED             # 24 % 4 == 0 but 256 % (24 / 4) != 0: not a vector-kernel shape
        else:
            assert call(0, 64, nv.BF16) == OK and call(0, 24, nv.F32) == OK
    if planes:      # row_map together with a residual / dres; a misaligned column parameter
        assert lib.u3d_bn_apply(h[0], h[1], h[2], h[3], h[4], h[7], 1, h[5], pl, h[6], 0, 64, nv.F32, h[8], None, None) == UNSUPPORTED
        assert lib.u3d_bn_bwd_apply(h[0], h[7], h[8], h[1], h[2], h[3], h[4], h[10], 1, h[5], h[11], pl, h[6], 0, 64, nv.F32, h[12], None) \
            == UNSUPPORTED
        odd = C.c_void_p(h[1].value + 4)
        assert lib.u3d_bn_apply(h[0], odd, h[2], h[3], h[4], None, 1, h[5], pl, h[6], 0, 64, nv.F32, None, None, None) == UNSUPPORTED
        assert lib.u3d_bn_bwd_apply(h[0], h[7], h[8], odd, h[2], h[3], h[4], h[10], 1, h[5], None, pl, h[6], 0, 64, nv.F32, None, None) \
            == UNSUPPORTED
