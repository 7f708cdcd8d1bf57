"""ctypes binding of libu3d_hip.so (C ABI declared in include/u3d_hip.h).

PyTorch is used only as the owner of device memory and streams: every call passes raw `data_ptr()`s and the
current HIP stream.  There is NO CPU fallback: if the library is missing or a call fails, we raise.

Signatures, struct layouts and constants are not restated here: abi.py reads them from the header, which therefore has to be on
disk next to the package (include/u3d_hip.h) wherever this module is imported.
"""
import collections
import ctypes as C
import os

import numpy as np
import torch

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("U3D_LIB_PATH") or os.path.join(_HERE, "libu3d_hip.so")      # override: kernel experiments (tools/build_variant.sh)

_ABI = abi.load()
_K = _ABI.constants


def _struct(c_name, py_name):
    return abi.structure(_ABI.structs[c_name], py_name)


def _slot_names(prefix):
    """The enumerators <prefix>* of the header in index order, without the prefix and the closing <prefix>COUNT."""
    names = sorted((v, n[len(prefix):]) for n, v in _K.items() if n.startswith(prefix))
    assert [v for v, _ in names] == list(range(len(names))) and names[-1][1] == "COUNT" and _K[prefix + "COUNT"] == len(names) - 1
    return [n for _, n in names[:-1]]


U3D_ERR_UNSUPPORTED = _K["U3D_ERR_UNSUPPORTED"]         # shape / dtype combination not compiled in: the caller takes another kernel
F32, BF16 = _K["U3D_F32"], _K["U3D_BF16"]


class U3DError(RuntimeError):
    pass


BitGridStruct = _struct("u3d_bitgrid", "BitGridStruct")

# DL_RPH0 .. DL_IOU2 and DL_NLIN, DL_NLN: the linears of a decoder layer (indices into DecLayerParams.w / .wt / .b); DLN_1 .. DLN_C2:
# its LayerNorms (.ln_g / .ln_b).  The header's two enums, under their names without the U3D_ prefix.
for _n, _v in _K.items():
    if _n.startswith(("U3D_DL_", "U3D_DLN_")):
        globals()[_n[4:]] = _v
DS_NAMES = _slot_names("U3D_DS_")       # forward-save slots of the fused decoder layer: SINE, RPH1, ... AMASK
DG_NAMES = _slot_names("U3D_DG_")       # its backward-workspace slots: CLSO, C2U, ... SINE
DecLayerParams = _struct("u3d_declayer_params", "DecLayerParams")
DecLayerDims = _struct("u3d_declayer_dims", "DecLayerDims")
WPackDesc = _struct("u3d_wpack_desc", "WPackDesc")
HaloTables = _struct("u3d_halo_tables", "HaloTables")

_lib = None
_I3 = C.c_int32 * 3     # the host arrays a few entry points take by pointer: constructors for the call sites
_F3 = C.c_float * 3
_F6 = C.c_float * 6


def exported_symbols():
    """Names every build of the library must export (checked by the CPU test-suite)."""
    return sorted(_ABI.prototypes)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise U3DError(f"{LIB_PATH} is missing: run `python -m uni3detr_amd.build` (hipcc, gfx950). "
                           "There is no CPU/PyTorch fallback for the HIP hot path.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _ABI.prototypes.items():
            fn = getattr(l, name)   # AttributeError -> loud failure if a symbol is missing
            fn.restype = res
            fn.argtypes = args
        if l.u3d_version() < 1:
            raise U3DError(f"{LIB_PATH} reports ABI version {l.u3d_version()}: rebuild it (python -m uni3detr_amd.build)")
        _lib = l
    return _lib


def _check(rc, what):
    if rc != 0:
        raise U3DError(f"{what} failed: {lib().u3d_strerror(rc).decode()} ({rc})")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device-contiguous tensor required"
    return C.c_void_p(t.data_ptr())


def dtype_code(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise U3DError(f"unsupported dtype {t.dtype}")


# --------------------------------------------------------------------------------------------------
# BitGrid
# --------------------------------------------------------------------------------------------------
class BitGrid:
    """Occupancy lattice of one sparse level (see include/u3d_hip.h)."""

    def __init__(self, batch, dims, device, linear=False):
        self.batch, self.dims = int(batch), tuple(int(d) for d in dims)
        self.linear = bool(linear)
        self.nwords = int(lib().u3d_bitgrid_nwords_layout(self.batch, *self.dims, 1 if linear else 0))
        self.words = torch.zeros(self.nwords, dtype=torch.int64, device=device)
        self.prefix = torch.empty(self.nwords + 1, dtype=torch.int32, device=device)
        self._scratch = torch.empty(int(lib().u3d_bitgrid_scan_scratch(self.nwords)), dtype=torch.int32, device=device)
        self.c = BitGridStruct(self.words.data_ptr(), self.prefix.data_ptr(), self.batch, *self.dims, 1 if linear else 0, 0)

    def set_row_capacity(self, cap):
        self.c.row_capacity = int(cap)

    def mark(self, coors):
        _check(lib().u3d_bitgrid_mark(C.byref(self.c), _ptr(coors), coors.shape[0], _stream()), "bitgrid_mark")

    def mark_strided(self, in_coors, n_dev, ksize, stride, pad):
        _check(lib().u3d_bitgrid_mark_strided(C.byref(self.c), _ptr(in_coors), _ptr(n_dev), in_coors.shape[0],
                                              _I3(*ksize), _I3(*stride), _I3(*pad), _stream()), "bitgrid_mark_strided")

    def scan(self):
        _check(lib().u3d_bitgrid_scan(C.byref(self.c), _ptr(self._scratch), _stream()), "bitgrid_scan")

    @property
    def count_dev(self):
        """int32 device scalar view: number of occupied cells (valid after scan())."""
        return self.prefix[self.nwords:]

    def rank(self, coors):
        out = torch.empty(coors.shape[0], dtype=torch.int32, device=coors.device)
        _check(lib().u3d_bitgrid_rank(C.byref(self.c), _ptr(coors), coors.shape[0], _ptr(out), _stream()), "bitgrid_rank")
        return out

    def coords(self, n):
        out = torch.empty((n, 4), dtype=torch.int32, device=self.words.device)      # (rows past the count: -1, written by the kernel)
        _check(lib().u3d_bitgrid_coords(C.byref(self.c), _ptr(out), n, _stream()), "bitgrid_coords")
        return out

    def scan_coords(self, n):
        """scan() + coords(n); in two launches where FUSED_SCAN_COORDS and the library's route allow (u3d_bitgrid_scan_coords)."""
        if not FUSED_SCAN_COORDS:
            self.scan()
            return self.coords(n)
        out = torch.empty((n, 4), dtype=torch.int32, device=self.words.device)
        _check(lib().u3d_bitgrid_scan_coords(C.byref(self.c), _ptr(self._scratch), _ptr(out), n, _stream()), "bitgrid_scan_coords")
        return out

    def nbr_table(self, q_coors, n_dev, ksize, stride, pad, mode):
        n = q_coors.shape[0]
        ld = (n + 127) // 128 * 128
        kvol = ksize[0] * ksize[1] * ksize[2]
        nbr = torch.empty((kvol, ld), dtype=torch.int32, device=q_coors.device)
        # route, decided here from host values: the 3x3x3 kernel on a block-major grid with 32-bit indices, else the generic one
        if (NBR_TABLE_K3 and tuple(ksize) == (3, 3, 3) and not self.linear and min(pad) >= 0 and self.nwords < 2 ** 31
                and 27 * ld < 2 ** 31):
            _check(lib().u3d_nbr_table_k3(C.byref(self.c), _ptr(q_coors), _ptr(n_dev), n, _I3(*stride), _I3(*pad), mode, _ptr(nbr), ld,
                                          _stream()), "nbr_table_k3")
            return nbr
        _check(lib().u3d_nbr_table(C.byref(self.c), _ptr(q_coors), _ptr(n_dev), n, _I3(*ksize), _I3(*stride), _I3(*pad),
                                   mode, _ptr(nbr), ld, _stream()), "nbr_table")
        return nbr


# A/B routes of the geometry build (tests/test_geometry_build_gpu.py runs both sides of each; no environment switch reads them)
NBR_TABLE_K3 = True          # 3x3x3 tables: 8 words + 8 prefixes loaded at once per row (False: the generic kernel, 54 dependent loads)
FUSED_SCAN_COORDS = True     # BitGrid.scan_coords in two launches (False: scan() + coords(), four)
VOX_CHUNK_RANKS = True       # voxelize_hard ranks over (scene, chunk) workgroups (False: one workgroup per scene + an offsets launch)


def dense_nbr_table(batch, q_dims, t_dims, ksize, stride, pad, mode, device):
    n = batch * q_dims[0] * q_dims[1] * q_dims[2]
    ld = (n + 127) // 128 * 128
    kvol = ksize[0] * ksize[1] * ksize[2]
    nbr = torch.empty((kvol, ld), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _check(lib().u3d_dense_nbr_table(batch, _I3(*q_dims), _I3(*t_dims), _I3(*ksize), _I3(*stride), _I3(*pad), mode, _ptr(nbr), ld,
                                         _stream()), "dense_nbr_table")
    return nbr


def active_nbr_table(coords, n_dev, batch, dims, tables):
    """Tables of a dense lattice restricted to a sparse level's active rows (u3d_active_nbr_table): for each int32 [K, ld] table
    of `tables` (one lattice [batch, dims], one K) -> int32 [K, ld_out] with t[k][i] = table[k][lattice row of coords[i]] for the
    level's rows i < *n_dev and -1 from there to ld_out = the capacity coords.shape[0] rounded up to 128.  One launch for all of them."""
    cap = coords.shape[0]
    ld_out = (cap + 127) // 128 * 128
    kvol, ld_src = tables[0].shape
    assert all(t.shape == tables[0].shape and t.dtype == torch.int32 and t.is_contiguous() for t in tables)
    out = torch.empty((len(tables), kvol, ld_out), dtype=torch.int32, device=coords.device)
    srcs = (C.c_void_p * len(tables))(*[t.data_ptr() for t in tables])
    _check(lib().u3d_active_nbr_table(_ptr(coords), _ptr(n_dev), cap, batch, _I3(*dims), srcs, len(tables), ld_src, kvol, _ptr(out),
                                      ld_out, _stream()), "active_nbr_table")
    return list(out.unbind(0))


# --------------------------------------------------------------------------------------------------
# voxelization
# --------------------------------------------------------------------------------------------------
def voxelize_hard(points, scene_off, batch, max_pts_per_scene, voxel_size, pc_range, max_points, max_voxels,
                  want_voxels=True, want_mean=True):
    """points f32 [n_total,F] (scenes concatenated), scene_off int32 [B+1] device.
    Returns (voxels|None, coors, num_points, mean|None, voxel_off) with capacity B*max_voxels rows."""
    n_total, nfeat = points.shape
    cap = batch * max_voxels
    dev = points.device
    voxels = torch.empty((cap, max_points, nfeat), dtype=torch.float32, device=dev) if want_voxels else None
    coors = torch.full((cap, 4), -1, dtype=torch.int32, device=dev)     # rows past the voxel count stay (-1,..): inert everywhere
    num = torch.zeros((cap,), dtype=torch.int32, device=dev)
    mean = torch.zeros((cap, nfeat), dtype=torch.float32, device=dev) if want_mean else None
    voxel_off = torch.empty((batch + 1,), dtype=torch.int32, device=dev)
    wsb = int(lib().u3d_voxelize_hard_workspace(n_total, batch, max_pts_per_scene))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    fn = lib().u3d_voxelize_hard_chunked if VOX_CHUNK_RANKS else lib().u3d_voxelize_hard
    _check(fn(_ptr(points), _ptr(scene_off), batch, n_total, max_pts_per_scene, nfeat,
              _F3(*voxel_size), _F6(*pc_range), max_points, max_voxels, _ptr(voxels), _ptr(coors),
              _ptr(num), _ptr(mean), _ptr(voxel_off), _ptr(ws), wsb, _stream()), "voxelize_hard")
    return voxels, coors, num, mean, voxel_off


def voxelize_dynamic(points, scene_off, batch, voxel_size, pc_range):
    """-> coors int32 [n_total,4] (b,z,y,x), (b,-1,-1,-1) for out-of-range points."""
    n_total, nfeat = points.shape
    coors = torch.empty((n_total, 4), dtype=torch.int32, device=points.device)
    _check(lib().u3d_voxelize_dynamic(_ptr(points), _ptr(scene_off), batch, n_total, nfeat, _F3(*voxel_size), _F6(*pc_range),
                                      _ptr(coors), _stream()), "voxelize_dynamic")
    return coors


def scatter_mean(points, rank, n_voxels):
    n_total, nfeat = points.shape
    sums = torch.zeros((n_voxels, nfeat), dtype=torch.float32, device=points.device)
    counts = torch.zeros((n_voxels,), dtype=torch.int32, device=points.device)
    _check(lib().u3d_scatter_mean(_ptr(points), _ptr(rank), n_total, nfeat, _ptr(sums), _ptr(counts), n_voxels, _stream()), "scatter_mean")
    return sums, counts


def scatter_mean_exact(points, rank, n_voxels):
    """scatter_mean with bits that do not depend on the order the points arrive in (u3d_scatter_mean_exact: fixed-point integer
    sums): -> (mean f32 [n_voxels, F], counts int32 [n_voxels]).  Nothing is zeroed here, nothing is read back."""
    n_total, nfeat = points.shape
    dev = points.device
    mean = torch.empty((n_voxels, nfeat), dtype=torch.float32, device=dev)
    counts = torch.empty((n_voxels,), dtype=torch.int32, device=dev)
    if n_voxels == 0:
        return mean, counts
    wsb = int(lib().u3d_scatter_mean_exact_workspace(n_voxels, nfeat))
    ws = torch.empty(wsb // 8 + 1, dtype=torch.int64, device=dev)           # 8-byte aligned
    _check(lib().u3d_scatter_mean_exact(_ptr(points), _ptr(rank), n_total, nfeat, _ptr(mean), _ptr(counts), n_voxels, _ptr(ws), ws.numel() * 8,
                                        _stream()), "scatter_mean_exact")
    return mean, counts


# --------------------------------------------------------------------------------------------------
# sparse conv / BN / dense
# --------------------------------------------------------------------------------------------------
class ExternalEvent:
    """HIP event recorded with hipEventRecordExternal on torch's current stream (torch.cuda.Event(external=True) is refused on
    ROCm builds): inside a capture it becomes an event-record node of the graph."""

    def __init__(self):
        h = C.c_void_p()
        _check(lib().u3d_event_create(C.byref(h)), "event_create")
        self.h = h

    def record(self):
        _check(lib().u3d_event_record(self.h, 1, _stream()), "event_record")

    def elapsed_time(self, other):
        ms = C.c_float()
        _check(lib().u3d_event_elapsed_ms(self.h, other.h, C.byref(ms)), "event_elapsed_ms")
        return float(ms.value)

    def __del__(self):
        try:
            lib().u3d_event_destroy(self.h)
        except Exception:
            pass


class KernelTimer:
    """HIP-event timing of individual launches on the stream they run on (used by bench.py for the roofline block).
    mode 'census': also counts the valid rulebook pairs P of each call (host sync) to price its algorithmic bytes:
    N_in*Cin*s + N_out*Cout*s + 8*P + K*Cin*Cout*s."""

    def __init__(self, mode="time", targets=(), per_step=0):
        """mode 'mark': only the calls whose index within the step (call counter modulo `per_step`) is in `targets` get events,
        and those are EXTERNAL events (hipEventRecordExternal): recorded inside a hipGraph capture they become event-record nodes
        of the graph, so after a replay `marks[i]` times that launch as it ran INSIDE the replayed step."""
        self.mode, self.calls, self.census = mode, [], []
        self.targets, self.per_step, self.counter, self.marks = set(targets), per_step, 0, {}

    def begin(self):
        if self.mode == "off":
            return None
        if self.mode == "mark":
            i = self.counter % self.per_step if self.per_step else self.counter
            self.counter += 1
            if i not in self.targets:
                return None
            try:
                e = ExternalEvent()
                e.record()
            except U3DError:                  # no event-record nodes on this runtime: keep the capture alive, time nothing
                self.mode, self.marks = "off", {}
                return None
            return (i, e)
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def end(self, tag, e0, meta=None):
        if self.mode == "off":
            return
        if self.mode == "mark":
            if e0 is not None:
                try:
                    e1 = ExternalEvent()
                    e1.record()
                    self.marks[e0[0]] = (tag, e0[1], e1)      # the latest recording wins: the captured one
                except U3DError:
                    self.mode, self.marks = "off", {}
            return
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        self.calls.append((tag, e0, e1))
        if self.mode == "census":
            self.census.append((tag, meta))

    def mark_durations_ms(self):
        """{index: ms} of the marked launches in the most recent (replayed) step."""
        torch.cuda.synchronize()
        return {i: a.elapsed_time(b) for i, (t, a, b) in self.marks.items()}

    def durations_ms(self):
        torch.cuda.synchronize()
        return [(t, a.elapsed_time(b)) for t, a, b in self.calls]


TIMER = None
CALL_KIND = "sparse"
USE_IGEMM_V2 = True


def census_meta(n_in, n_out, cin, cout, kvol, nbr, act_bytes=2, w_bytes=None, v2=True, split=False, in_bytes=None):
    """The census entry of one convolution launch: its valid rulebook pairs P (counted from `nbr`: a table, a RevNbr - reversing the
    offsets does not change the count - or None for a plain row product, P = n_out; one host sync) and its algorithmic bytes
    N_in*Cin*s + N_out*Cout*s + 8*P + K*Cin*Cout*w, s / w = bytes per activation / weight element (w_bytes=None: as the
    activations; a weight gradient is written in f32: 4).  in_bytes: bytes per INPUT element where they differ from the output's (an fp8
    launch reads e4m3 rows and writes bf16 rows); None: act_bytes.
    split: a split-bf16 launch (kvol = the offsets of ONE of its three products) is priced as the f32 convolution it stands for: f32
    rows in and out, f32 weights, 2 * pairs * cin * cout flops (the kernel issues 3x)."""
    if split:
        act_bytes = w_bytes = 4
    elif w_bytes is None:
        w_bytes = act_bytes
    if in_bytes is None or split:
        in_bytes = act_bytes
    tab = nbr.t if isinstance(nbr, RevNbr) else nbr
    pairs = n_out if tab is None else int((tab[:kvol, :n_out] >= 0).sum().item())
    meta = dict(kind=CALL_KIND, v2=v2, split=True) if split else dict(kind=CALL_KIND, v2=v2)
    meta.update(n_in=n_in, n_out=n_out, cin=cin, cout=cout, kvol=kvol, pairs=pairs,
                bytes=n_in * cin * in_bytes + n_out * cout * act_bytes + 8 * pairs + kvol * cin * cout * w_bytes, flops=2 * pairs * cin * cout)
    return meta


def timed_begin():
    """Opens the timed region of one launch: exactly one TIMER.begin() (bench.py's "mark" mode indexes launches by that counter).
    -> None when no timer is installed (nothing is recorded then; a wrapper on the step's host path skips its timed_end call
    altogether), else what timed_end() takes."""
    t = TIMER
    return None if t is None else (t, t.begin())


def timed_end(region, tag, *shape, **price):
    """Closes the region under `tag`; shape / price: census_meta's arguments, evaluated in census mode only (the pair count reads the
    device).  A launch that raised never gets here: no end() is recorded for it."""
    if region is not None:
        t, e0 = region
        t.end(tag, e0, census_meta(*shape, **price) if (shape and t.mode == "census") else None)


# The forward launch plan (fwd_plan in csrc/igemm_bf16.hip), as u3d_igemm_fwd_plan reports it: the kernel family, the kernel's name
# within it, its tile, the statistics layout of a "stats" launch and whether the kernel's epilogue takes the addend.
FWD_EPI = {n.lower(): i for i, n in enumerate(_slot_names("U3D_FWD_EPI_"))}      # plain, add, stats, affine
FWD_FAMILIES = tuple(n.lower() for n in _slot_names("U3D_FWD_FAM_"))             # none, conv_in, direct, glds, reg
AFFINE_KERNELS = ("glds_256x256", "glds8_256x256", "glds8_192x256", "glds8_256x128", "glds8_192x128", "glds_256x128", "glds_128x128",
                  "glds_128x64")
FWD_KERNELS = {"conv_in": ("conv_in",), "glds": AFFINE_KERNELS,
               # <padded cin>x<cout>_<k-major | n-major | n-major + statistics | n-major f32 output>
               "direct": tuple(f"{s}_{v}" for s in ("32x16", "32x32", "32x64", "64x16", "64x32") for v in ("k", "n", "ns", "nf")),
               "reg": ("n16_k", "n16_n", "n32_k", "n32_n", "n64_k", "n64_n", "256x256", "256x128", "128x64")}
FwdPlanInfo = _struct("u3d_fwd_plan_info", "FwdPlanInfo")
FwdPlan = collections.namedtuple("FwdPlan", "family kernel rows cols partials rows_per_partial takes_addend")


def fwd_plan(n_out, cin, cout, kvol, has_nbr, nmajor, epi="plain"):
    """The kernel u3d_igemm_fwd_bf16 (epi "plain" / "add" / "stats") or u3d_igemm_fwd_affine_bf16 ("affine") takes for the shape, None
    when no implicit-GEMM kernel serves it (with "stats": none with a statistics epilogue).  Asked with "add" for a kernel without an
    addend epilogue, the answer is the plain plan with takes_addend False.  Host only: the library answers without a GPU."""
    i = FwdPlanInfo()
    rc = lib().u3d_igemm_fwd_plan(n_out, cin, cout, kvol, bool(has_nbr), bool(nmajor), FWD_EPI[epi], C.byref(i))
    if rc:
        return None if rc == U3D_ERR_UNSUPPORTED else _check(rc, "igemm_fwd_plan")
    family = FWD_FAMILIES[i.family]
    return FwdPlan(family, FWD_KERNELS[family][i.kernel], i.rows, i.cols, i.partials, i.rows_per_partial, bool(i.takes_addend))


def fwd_stats_layout(n_out, cin, cout, kvol, has_nbr):
    """(partials, rows per partial) of the statistics a "stats" launch with n-major weights writes for this shape, None when no kernel
    with a statistics epilogue serves it.  Rows 0: one partial per wave of the direct-operand kernels, all of them count (rows_per_block
    = 0 downstream).  u3d_igemm_fwd_split_bf16 writes the same layout wherever it serves the shape."""
    p = fwd_plan(n_out, cin, cout, kvol, has_nbr, True, "stats")
    return p and (p.partials, p.rows_per_partial)


class SubmHalo:
    """Per-tile distinct-row lists + 16-bit slot tables of one SubM level (u3d_subm_halo_build): built once per level and step from
    the forward neighbour table, shared by all of the level's 64 -> 64 convs and (offsets reversed) their input gradients."""
    TILE = 128

    MAX_ROWS = 140 * 256 * 32       # u3d_subm_halo_build's LDS row bitmap: 4.5 B per 32 rows + 1 KiB within 160 KiB (the C side decides)

    def __init__(self, nbr_fwd, n_dev, n_cap):
        dev = nbr_fwd.device
        a, b, t = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        _check(lib().u3d_subm_halo_sizes(n_cap, C.byref(a), C.byref(b), C.byref(t)), "subm_halo_sizes")
        self.tiles, self.n_dev, self.n_cap, self.nbr = t.value, n_dev, n_cap, nbr_fwd
        self.kvol = nbr_fwd.shape[0]                     # <= 27 offsets (27: sparse SubM levels; 9: the dense stack's (1,3,3) convs)
        self.tile_rows = torch.empty((a.value,), dtype=torch.int32, device=dev)
        self.loc = torch.empty((b.value,), dtype=torch.int16, device=dev)
        self.tile_cnt = torch.empty((t.value,), dtype=torch.int32, device=dev)
        # what every entry that reads the tables takes (by reference); the tensors above keep the memory alive
        self.tables = HaloTables(self.tile_rows.data_ptr(), self.loc.data_ptr(), self.tile_cnt.data_ptr(), n_dev.data_ptr(), n_cap, self.kvol)
        rc = lib().u3d_subm_halo_build(_ptr(nbr_fwd), nbr_fwd.shape[1], _ptr(n_dev), n_cap, _ptr(self.tile_rows), _ptr(self.loc),
                                       _ptr(self.tile_cnt), self.kvol, _stream())
        self.ok = rc != U3D_ERR_UNSUPPORTED     # more rows than the LDS row bitmap holds - the caller keeps the table kernels
        if self.ok:
            _check(rc, "subm_halo_build")


def subm_halo_wgrad(x, dy, halo, out=None, max_slots=0):
    """dW f32 [27, 64, 64] of a 64 -> 64 SubM conv from the level's halo tables (u3d_subm_halo_wgrad64_bf16); out: contiguous f32
    tensor of 27 * 64 * 64 elements to write into."""
    assert x.dtype == torch.bfloat16 and dy.dtype == torch.bfloat16 and x.shape == dy.shape == (halo.n_cap, 64)
    dw = out.view(27, 64, 64) if (out is not None and out.is_contiguous() and out.dtype == torch.float32 and out.numel() == 27 * 4096) \
        else torch.empty((27, 64, 64), dtype=torch.float32, device=x.device)
    wsb = int(lib().u3d_subm_halo_wgrad64_workspace())
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    region = timed_begin()
    _check(lib().u3d_subm_halo_wgrad64_bf16(_ptr(x), _ptr(dy), C.byref(halo.tables), _ptr(dw), _ptr(ws), wsb, int(max_slots), _stream()),
           "subm_halo_wgrad64_bf16")
    if region is not None:
        timed_end(region, "spconv_wgrad", halo.n_cap, halo.n_cap, 64, 64, 27, halo.nbr, w_bytes=4)
    return dw


def subm_halo_wpack(w_nmajor, out=None):
    """bf16 [27, 64 (out), 64 (reduction)] / [kvol, 128, 128] -> the MFMA fragment order u3d_subm_halo_conv_bf16 reads (same shape and
    size)."""
    k, c = w_nmajor.shape[0], w_nmajor.shape[1]
    assert w_nmajor.dtype == torch.bfloat16 and w_nmajor.is_contiguous() and w_nmajor.shape[2] == c
    assert (k == 27 and c == 64) or (1 <= k <= 27 and c == 128)
    out = torch.empty_like(w_nmajor) if out is None else out
    _check(lib().u3d_subm_halo_wpack(_ptr(w_nmajor), _ptr(out), c, k, _stream()), "subm_halo_wpack")
    return out


HaloWpackPlan = collections.namedtuple("HaloWpackPlan", "src dst n pairs c kvol")      # src / dst: device pointer arrays; pairs: kept alive


def subm_halo_wpack_plan(pairs, device):
    """[(src, dst)] of [27, C, C] bf16 tensors, all with the same C in (64, 128) -> plan for subm_halo_wpack_batched (device pointer
    arrays; the tensors must stay alive)."""
    k, c = pairs[0][0].shape[0], pairs[0][0].shape[1]
    assert all(tuple(a.shape) == (k, c, c) for a, _ in pairs) and ((k == 27 and c == 64) or c == 128)
    src = torch.tensor([a.data_ptr() for a, _ in pairs], dtype=torch.int64, device=device)
    dst = torch.tensor([b.data_ptr() for _, b in pairs], dtype=torch.int64, device=device)
    return HaloWpackPlan(src, dst, len(pairs), pairs, c, k)


def subm_halo_wpack_batched(plan):
    _check(lib().u3d_subm_halo_wpack_batched(_ptr(plan.src), _ptr(plan.dst), plan.n, plan.c, plan.kvol, _stream()), "subm_halo_wpack_batched")


def subm_halo_conv(inp, w_packed, halo, krev=False, addend=None, want_stats=False, tag="spconv_fwd", max_slots=0):
    """64 -> 64 channel, 27-offset (or 128 -> 128, <= 27-offset) SubM conv out of the tile's staged distinct rows
    (u3d_subm_halo_conv_bf16 without a shift).  w_packed: subm_halo_wpack of bf16 [kvol, C (out), C (reduction)].  -> out, or (out, stats f64 [tiles, 2, 64], 128) with want_stats."""
    c = inp.shape[1]
    assert inp.dtype == torch.bfloat16 and c in (64, 128) and tuple(w_packed.shape) == (halo.kvol, c, c) and inp.shape[0] == halo.n_cap
    assert c == 128 or halo.kvol == 27
    out = torch.empty_like(inp)
    stats = torch.empty((halo.tiles, 2, c), dtype=torch.float64, device=inp.device) if want_stats else None
    region = timed_begin()
    _check(lib().u3d_subm_halo_conv_bf16(_ptr(inp), _ptr(w_packed), C.byref(halo.tables), c, int(krev), _ptr(addend), _ptr(out), _ptr(stats),
                                         None, 0, int(max_slots), _stream()), "subm_halo_conv_bf16")
    if region is not None:
        timed_end(region, tag, halo.n_cap, halo.n_cap, c, c, halo.kvol, halo.nbr)
    return (out, stats, SubmHalo.TILE) if want_stats else out


def subm_halo_conv_affine(inp, w_packed, halo, shift, relu, addend=None, max_slots=0, out=None, tag="spconv_fwd"):
    """act(conv(inp) + shift + addend) of a 64 -> 64 / 128 -> 128 SubM conv whose eval-mode BatchNorm is folded into the weights, out
    of the level's halo tables in one launch (u3d_subm_halo_conv_bf16 with a shift).  w_packed: subm_halo_wpack of
    the FOLDED n-major weights (bn_fold), shift f32 [C], addend bf16 [n, C] or None (the residual block's identity).  Rows at or past
    *halo.n_dev of `out` are left as they are."""
    c = inp.shape[1]
    assert inp.dtype == torch.bfloat16 and c in (64, 128) and tuple(w_packed.shape) == (halo.kvol, c, c) and inp.shape[0] == halo.n_cap
    assert w_packed.dtype == torch.bfloat16 and (c == 128 or halo.kvol == 27)
    assert shift.dtype == torch.float32 and tuple(shift.shape) == (c,) and shift.data_ptr() % 16 == 0
    assert addend is None or (addend.dtype == torch.bfloat16 and addend.shape == inp.shape)
    if out is None:
        out = torch.empty_like(inp)
    assert out.shape == inp.shape and out.dtype == torch.bfloat16
    region = timed_begin()
    _check(lib().u3d_subm_halo_conv_bf16(_ptr(inp), _ptr(w_packed), C.byref(halo.tables), c, 0, _ptr(addend), _ptr(out), None, _ptr(shift),
                                         int(bool(relu)), int(max_slots), _stream()), "subm_halo_conv_bf16")
    if region is not None:
        timed_end(region, tag, halo.n_cap, halo.n_cap, c, c, halo.kvol, halo.nbr)
    return out


def bn_finalize_partials(stats, tile_rows, n_dev, n_cap, eps, momentum, running_mean=None, running_var=None, num_batches=None):
    nblocks, _, c = stats.shape
    mean = torch.empty((c,), dtype=torch.float32, device=stats.device)
    invstd = torch.empty((c,), dtype=torch.float32, device=stats.device)
    _check(lib().u3d_bn_finalize_partials(_ptr(stats), nblocks, tile_rows, _ptr(n_dev), n_cap, c, eps, momentum, _ptr(running_mean),
                                          _ptr(running_var), _ptr(num_batches), _ptr(mean), _ptr(invstd), _stream()), "bn_finalize_partials")
    return mean, invstd


class RevNbr:
    """A neighbour table read with its offsets in REVERSED order (row K-1-k for offset k): what the transposed table of a
    submanifold convolution is - voxel j is the neighbour of m at offset +d exactly when m is the neighbour of j at -d, and the
    3x3x3 offsets are enumerated symmetrically.  Handed to the kernels as a pointer to the last table row with a negative row
    stride: the input gradient of a SubM layer needs no table of its own (4 table builds per step less)."""

    def __init__(self, table):
        self.t = table
        self.shape = table.shape

    def ptr_ld(self):
        k, ld = self.t.shape
        return C.c_void_p(self.t.data_ptr() + (k - 1) * ld * 4), -ld


def _nbr_ptr_ld(nbr):
    if nbr is None:
        return _ptr(None), 0
    if isinstance(nbr, RevNbr):
        return nbr.ptr_ld()
    return _ptr(nbr), nbr.shape[1]


def spconv_fwd(inp, w, nbr, n_out_dev, n_out, cout, transpose_w=False, tag=None, addend=None, want_stats=False):
    """out[m] = sum_k in[nbr[k][m]] @ W[k]; w: [K, Cin_w, Cout_w] contiguous. Returns [n_out, cout].  nbr may be a RevNbr.
    addend (bf16 [n_out, cout], optional): summed into the result - by the kernel's epilogue where it has one, else afterwards.
    want_stats: -> (out, stats, rows per partial), stats = the BatchNorm statistics of the output per row tile or wave, f64 [partials, 2,
    cout], or None where no kernel with a statistics epilogue serves the shape (they need n-major weights: transpose_w).
    One plan query (two when statistics are wanted and not to be had), one launch: the plan's implicit-GEMM kernel, or the
    first-generation kernel where there is none (small or odd channel counts, f32)."""
    assert addend is None or not want_stats
    kvol = w.shape[0]
    cin = inp.shape[1]
    out = torch.empty((n_out, cout), dtype=inp.dtype, device=inp.device)
    nbr_p, ld = _nbr_ptr_ld(nbr)
    tw = 1 if transpose_w else 0
    plan = stats = None
    fused = False                          # the launch takes the addend: in f32 before the one rounding (afterwards rounds twice)
    if inp.dtype == torch.bfloat16 and USE_IGEMM_V2:
        if want_stats:
            plan = fwd_plan(n_out, cin, cout, kvol, ld != 0, tw, "stats")
            if plan is not None and plan.partials:
                stats = torch.empty((plan.partials, 2, cout), dtype=torch.float64, device=inp.device)
        if stats is None:
            fused = addend is not None and ld != 0 and addend.dtype == torch.bfloat16 and addend.shape == out.shape and addend.is_contiguous()
            plan = fwd_plan(n_out, cin, cout, kvol, ld != 0, tw, "add" if fused else "plain")
            fused = fused and plan is not None and plan.takes_addend
    region = timed_begin()
    if plan is not None:
        _check(lib().u3d_igemm_fwd_bf16(_ptr(inp), _ptr(w), nbr_p, ld, _ptr(out), _ptr(n_out_dev), n_out, cin, cout, kvol, tw,
                                        _ptr(addend) if fused else None, _ptr(stats), _stream()), "igemm_fwd_bf16")
    else:
        _check(lib().u3d_spconv_fwd(_ptr(inp), _ptr(w), nbr_p, ld, _ptr(out), _ptr(n_out_dev), n_out, cin, cout, kvol, tw,
                                    dtype_code(inp), _stream()), "spconv_fwd")
    if region is not None:
        timed_end(region, tag or ("spconv_dgrad" if transpose_w else "spconv_fwd"), inp.shape[0], n_out, cin, cout, kvol, nbr,
                  act_bytes=inp.element_size(), v2=plan is not None)
    if addend is not None and not fused:
        out += addend
    return (out, stats, plan.rows_per_partial if stats is not None else 0) if want_stats else out


def split_rows(x, n_dev, n_cap=None):
    """f32 [n_cap, c] -> bf16 [2 * n_cap, c]: hi plane = bf16(x), lo plane = bf16(x - hi) (u3d_split_rows_f32).  Rows between the
    device-side count and n_cap are written as ZEROS in both planes (the kernel zero-fills up to the capacity: the LDS-DMA kernels stage
    whole tiles, and a NaN bit pattern in a never-named padding row would still poison a BatchNorm statistic through 0 * NaN)."""
    n_cap = x.shape[0] if n_cap is None else n_cap
    assert x.dtype == torch.float32 and x.is_contiguous()
    out = torch.empty((2 * n_cap, x.shape[1]), dtype=torch.bfloat16, device=x.device)
    _check(lib().u3d_split_rows_f32(_ptr(x), _ptr(n_dev), n_cap, x.shape[1], _ptr(out), _stream()), "split_rows_f32")
    return out


def direct_serves(cin, cout, kvol):
    """The shapes of the direct-operand kernels (igemm_direct.hip, u3d_plan_igemm_direct): 27 offsets, 16 / 32 / 64 channels, not
    64 -> 64."""
    return kvol == 27 and cin in (16, 32, 64) and cout in (16, 32, 64) and not (cin == 64 and cout == 64)


def spconv_fwd_split_direct(xs, w3, nbr, n_out_dev, n_out, cout, tag="spconv_fwd"):
    """Split-bf16 product on a narrow 27-offset level (u3d_igemm_direct_split_bf16): xs bf16 planes [2 * n_in, cin], w3 bf16
    [81, cout, cin] = (wh, wl, wh), nbr the PLAIN table (or a RevNbr) -> f32 [n_out, cout]."""
    cin, n_in = xs.shape[1], xs.shape[0] // 2
    out = torch.empty((n_out, cout), dtype=torch.float32, device=xs.device)
    nbr_p, ld = _nbr_ptr_ld(nbr)
    region = timed_begin()
    _check(lib().u3d_igemm_direct_split_bf16(_ptr(xs), _ptr(w3), nbr_p, ld, _ptr(out), _ptr(n_out_dev), n_out, n_in, cin, cout, _stream()),
           "igemm_direct_split_bf16")
    if region is not None:
        timed_end(region, tag, n_in, n_out, cin, cout, 27, nbr, split=True)
    return out


_SplitRowsJobs = _struct("U3dSplitRowsJobs", "_SplitRowsJobs")


def split_rows_batch_into(tensors, outs):
    """hi / lo bf16 planes of several f32 row matrices (2-D, unit column stride, any row stride) in one launch per 32 of them
    (u3d_split_rows_batch); outs[i]: bf16 [2 * rows, cols] (hi plane, then lo plane), written here."""
    for i in range(0, len(tensors), 32):
        jobs = _SplitRowsJobs()
        chunk = list(zip(tensors[i:i + 32], outs[i:i + 32]))
        jobs.njobs = len(chunk)
        for j, (t, o) in enumerate(chunk):
            assert t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.shape[1] % 4 == 0 and t.stride(0) % 4 == 0
            assert o.dtype == torch.bfloat16 and o.is_contiguous() and tuple(o.shape) == (2 * t.shape[0], t.shape[1])
            jobs.src[j], jobs.dst[j] = t.data_ptr(), o.data_ptr()
            jobs.ld[j], jobs.rows[j], jobs.cols[j] = t.stride(0), t.shape[0], t.shape[1]
        _check(lib().u3d_split_rows_batch(C.byref(jobs), _stream()), "split_rows_batch")


def split_rows_batch(tensors):
    outs = [torch.empty((2 * t.shape[0], t.shape[1]), dtype=torch.bfloat16, device=t.device) for t in tensors]
    split_rows_batch_into(tensors, outs)
    return outs


def sum3(a, b, c):
    """(a + b) + c for three contiguous f32 tensors of one shape, one launch (u3d_sum3_f32)."""
    assert a.shape == b.shape == c.shape and a.dtype == b.dtype == c.dtype == torch.float32
    a, b, c = a.contiguous(), b.contiguous(), c.contiguous()
    if a.numel() % 4 != 0 or not a.is_cuda:
        return a + b + c
    out = torch.empty_like(a)
    _check(lib().u3d_sum3_f32(_ptr(a), _ptr(b), _ptr(c), _ptr(out), a.numel(), _stream()), "sum3_f32")
    return out


def _split3_geometry(w, layout, nmajor):
    """(k, a, b, sk, sa, sb): the [K, A, B] view of a conv parameter in its checkpoint layout, as element strides."""
    if layout == "dhwio":
        kd, kh, kw, cin, cout = w.shape
        k = kd * kh * kw
        sk, s_ci, s_co = cin * cout, cout, 1
    else:
        cout, cin, kd, kh, kw = w.shape
        k = kd * kh * kw
        sk, s_ci, s_co = 1, k, cin * k
    a, b, sa, sb = (cout, cin, s_co, s_ci) if nmajor else (cin, cout, s_ci, s_co)
    return k, a, b, sk, sa, sb


def _upload_jobs(jobs, device):
    """A ctypes array of job records as a device byte tensor (the caller keeps it alive for as long as a launch may read it)."""
    return torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(device)


class Split3Set:
    """Every (conv parameter, layout, n-major?) triple a step asks for, refreshed by ONE launch at the top of the step
    (u3d_split3_weights_batch).  A request the set has not seen yet is served by its own launch and joins the set; entries whose
    parameter died or moved (TrainStep re-homes parameters into its flat buffer) are dropped / re-described at the next refresh."""

    _Job = _struct("u3d_split3_job", "_Job")

    def __init__(self):
        self.entries = {}            # (data_ptr, nmajor) -> [weakref, layout, nmajor, dst, data_ptr, in the job table?, version, shape]
        self.jobs_dev = None
        self._keep = []              # every job table ever uploaded: a captured graph may still read an older one
        self.total_blocks = 0
        self.dirty = True
        self.fresh = False           # the dst tensors hold the split of the CURRENT parameter values

    def get(self, weight, layout, nmajor):
        """Keyed by the parameter's MEMORY (the backward sees the saved tensor, not necessarily the Parameter object)."""
        e = self.entries.get((weight.data_ptr(), bool(nmajor)))
        if e is not None and e[0]() is not None and e[1] == layout and e[7] == tuple(weight.shape):
            # served only when THIS step's refresh computed it from the parameter's current values (in-place torch updates bump the
            # version; TrainStep's flat AdamW does not, but every step of it starts with a refresh)
            if self.fresh and e[5] and e[6] == weight._version:
                return e[3]
        return None

    def add(self, weight, layout, nmajor, dst):
        import weakref
        key = (weight.data_ptr(), bool(nmajor))
        old = self.entries.get(key)
        if old is not None and old[0]() is not None and old[1] == layout and old[7] == tuple(weight.shape) and old[5]:
            return                    # already in the job table (asked for before this step's refresh could serve it)
        self.entries[key] = [weakref.ref(weight), layout, bool(nmajor), dst, weight.data_ptr(), False, -1, tuple(weight.shape)]
        self.dirty = True

    def refresh(self):
        """One launch over every live entry (called at the top of a step's forward, inside the captured graph too - the job table is
        rebuilt on the host only OUTSIDE a capture; a table that went stale during one falls back to per-request launches)."""
        dead = [k for k, e in self.entries.items() if e[0]() is None]
        for k in dead:
            del self.entries[k]
            self.dirty = True
        moved = [k for k, e in self.entries.items() if e[0]().data_ptr() != e[4]]      # re-homed parameters (TrainStep's flat buffer): asked for again
        for k in moved:
            del self.entries[k]
            self.dirty = True
        if not self.entries:
            self.fresh = False
            return
        if self.dirty:
            if torch.cuda.is_current_stream_capturing():
                self.fresh = False
                return
            assert int(lib().u3d_split3_job_bytes()) == C.sizeof(Split3Set._Job)
            jobs = (Split3Set._Job * len(self.entries))()
            fb = 0
            for j, e in enumerate(self.entries.values()):
                w = e[0]().detach()
                k, a, b, sk, sa, sb = _split3_geometry(w, e[1], e[2])
                jobs[j].src, jobs[j].dst = w.data_ptr(), e[3].data_ptr()
                jobs[j].sk, jobs[j].sa, jobs[j].sb = sk, sa, sb
                jobs[j].K, jobs[j].A, jobs[j].B, jobs[j].first_block = k, a, b, fb
                fb += int(lib().u3d_split3_job_blocks(k, a, b))
                e[5] = True
            self.jobs_dev = _upload_jobs(jobs, next(iter(self.entries.values()))[3].device)
            self._keep.append(self.jobs_dev)
            self.total_blocks, self.njobs, self.dirty = fb, len(self.entries), False
        _check(lib().u3d_split3_weights_batch(_ptr(self.jobs_dev), self.njobs, self.total_blocks, _stream()), "split3_weights_batch")
        for e in self.entries.values():
            e[6] = e[0]()._version
        self.fresh = True


SPLIT3_DEFAULT = Split3Set()   # scopes without an owner (ad-hoc calls, tests); a detector brings its own set (detector.stage_features)
SPLIT3_ACTIVE = None           # the set of the split scope being executed (sparse.split_scope), None outside
SPLIT3_BATCH = True            # test-only module attribute: False = one u3d_split3_weights launch per request (the A/B formulation)


def split3_weights(weight, layout, nmajor, cache=None):
    """Conv PARAMETER (f32, checkpoint layout "dhwio" [kD,kH,kW,Cin,Cout] or "oidhw" [Cout,Cin,kD,kH,kW]) -> bf16 [3K, A, B] = (hi, lo, hi)
    of its [K, Cout, Cin] (nmajor) or [K, Cin, Cout] view, read in place through element strides (u3d_split3_weights) - or, when the
    step's batched refresh (Split3Set) already produced it, the cached tensor."""
    cache = cache if cache is not None else SPLIT3_ACTIVE
    if not (SPLIT3_BATCH and weight.is_cuda):
        cache = None
    if cache is not None:
        hit = cache.get(weight, layout, nmajor)
        if hit is not None:
            return hit
    w = weight.detach()
    assert w.dtype == torch.float32 and w.is_contiguous() and w.dim() == 5
    k, a, b, sk, sa, sb = _split3_geometry(w, layout, nmajor)
    out = torch.empty((3 * k, a, b), dtype=torch.bfloat16, device=w.device)
    _check(lib().u3d_split3_weights(_ptr(w), sk, sa, sb, k, a, b, _ptr(out), _stream()), "split3_weights")
    # only PARAMETERS join the set: a temporary (the FPN's transposed-conv weights reach here as a re-laid-out copy made each step) has
    # new memory every time - its entry would be pruned and re-added at every refresh and keep the job table dirty for ever
    if cache is not None and isinstance(weight, torch.nn.Parameter) and not torch.cuda.is_current_stream_capturing():
        cache.add(weight, layout, nmajor, out)
    return out


# --------------------------------------------------------------------------------------------------
# Inference: eval-mode BatchNorm folded into the convolution in front of it (csrc/bn_fold.hip, u3d_igemm_fwd_affine_bf16)
# --------------------------------------------------------------------------------------------------
BnFoldJob = _struct("u3d_bn_fold_job", "BnFoldJob")       # one record of u3d_bn_fold_batched's device job table


def conv_weight_strides(shape, layout):
    """(kvol, cout, cin, sk, sa, sb) of a conv parameter of `shape` in its checkpoint layout ("dhwio" [kD,kH,kW,Cin,Cout] / "oidhw"
    [Cout,Cin,kD,kH,kW]): element (k, co, ci) lies at k * sk + co * sa + ci * sb."""
    if layout == "dhwio":
        kd, kh, kw, cin, cout = shape
        k = kd * kh * kw
        return k, cout, cin, cin * cout, 1, cout
    if layout != "oidhw":
        raise ValueError(f"unknown conv weight layout {layout!r}")
    cout, cin, kd, kh, kw = shape
    k = kd * kh * kw
    return k, cout, cin, 1, cin * k, k


def bn_fold_job_table(specs):
    """Host side of the job table.  specs: dicts with w / gamma / beta / mean / var / w_folded / shift (addresses; shift None with
    scale_only), shape + layout of the master weight, eps, scale_only.  -> (ctypes array of BnFoldJob, total blocks of the launch)."""
    assert int(lib().u3d_bn_fold_job_bytes()) == C.sizeof(BnFoldJob)
    jobs = (BnFoldJob * len(specs))()
    fb = 0
    for j, sp in zip(jobs, specs):
        k, cout, cin, sk, sa, sb = conv_weight_strides(tuple(sp["shape"]), sp["layout"])
        if cin % 4:
            raise U3DError(f"bn_fold: Cin = {cin} is not a multiple of 4")
        so = int(bool(sp.get("scale_only", False)))
        if not so and not sp.get("shift"):
            raise U3DError("bn_fold: a job that is not scale_only needs a shift buffer")
        j.w, j.gamma, j.beta, j.mean, j.var = sp["w"], sp["gamma"], sp["beta"], sp["mean"], sp["var"]
        j.w_folded, j.shift = sp["w_folded"], sp.get("shift") or None
        j.sk, j.sa, j.sb, j.eps = sk, sa, sb, float(sp["eps"])
        j.kvol, j.cout, j.cin, j.scale_only, j.first_block = k, cout, cin, so, fb
        fb += int(lib().u3d_bn_fold_job_blocks(k, cout, cin))
    return jobs, fb


class _FoldTable:
    """A fold job table on the device + what it points at (kept alive).  run(): ONE launch over every pair (ENTRY).  pairs: (weight
    f32 parameter, layout, gamma, beta, running_mean, running_var (f32 [Cout] each), eps, destinations ...); a subclass checks the
    destinations and fills the records in _jobs(pairs, geo) -> (ctypes array, total blocks), geo[i] = conv_weight_strides of pair i."""

    def __init__(self, pairs):
        geo = []
        for w, layout, gamma, beta, mean, var, *_ in pairs:
            geo.append(conv_weight_strides(tuple(w.shape), layout))
            for t in (w, gamma, beta, mean, var):
                assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), self.ENTRY[4:] + " reads contiguous f32 device tensors"
            assert all(tuple(t.shape) == (geo[-1][1],) for t in (gamma, beta, mean, var))
        jobs, self.total_blocks = self._jobs(pairs, geo)
        self.njobs, self.pairs = len(pairs), list(pairs)
        self.jobs_dev = _upload_jobs(jobs, pairs[0][7].device)

    def run(self):
        _check(getattr(lib(), self.ENTRY)(_ptr(self.jobs_dev), self.njobs, self.total_blocks, _stream()), self.ENTRY[4:])


class BnFoldTable(_FoldTable):
    """destinations: w_folded bf16 [kvol, Cout, Cin], shift f32 [Cout] or None = scale_only."""
    ENTRY = "u3d_bn_fold_batched"

    def _jobs(self, pairs, geo):
        specs = []
        for (w, layout, gamma, beta, mean, var, eps, wf, shift), (k, cout, cin, *_) in zip(pairs, geo):
            assert wf.is_cuda and wf.dtype == torch.bfloat16 and wf.is_contiguous() and tuple(wf.shape) == (k, cout, cin)
            assert shift is None or (shift.is_cuda and shift.dtype == torch.float32 and tuple(shift.shape) == (cout,))
            specs.append(dict(w=w.data_ptr(), gamma=gamma.data_ptr(), beta=beta.data_ptr(), mean=mean.data_ptr(), var=var.data_ptr(),
                              w_folded=wf.data_ptr(), shift=None if shift is None else shift.data_ptr(), shape=w.shape, layout=layout,
                              eps=eps, scale_only=shift is None))
        return bn_fold_job_table(specs)


def bn_fold(pairs):
    """Fold every (conv weight, BatchNorm) pair in one launch; -> the BnFoldTable (run() folds again after the sources changed)."""
    t = BnFoldTable(pairs)
    t.run()
    return t


def igemm_fwd_affine_plan(n_out, cin, cout, kvol, has_nbr):
    """(kernel name, tile rows, tile columns) u3d_igemm_fwd_affine_bf16 takes for the shape; None when it does not serve it."""
    p = fwd_plan(n_out, cin, cout, kvol, has_nbr, True, "affine")
    return p and (p.kernel, p.rows, p.cols)


def igemm_fwd_affine(inp, w_folded, nbr, shift, relu, n_out_dev, n_out, out=None, tag="spconv_fwd"):
    """out = act(conv(inp; w_folded) + shift): conv -> eval BatchNorm (-> ReLU) in one launch (u3d_igemm_fwd_affine_bf16).  inp bf16
    [n_in, cin], w_folded bf16 [kvol, cout, cin] (bn_fold), nbr int32 [kvol, ld] or None for kvol == 1, shift f32 [cout].  Rows at or
    past *n_out_dev of `out` are left as they are.  A shape the entry does not serve is an error: there is no other route."""
    kvol, cout, cin = w_folded.shape
    assert inp.dtype == torch.bfloat16 and w_folded.dtype == torch.bfloat16 and shift.dtype == torch.float32
    assert inp.shape[1] == cin and tuple(shift.shape) == (cout,) and (nbr is not None or kvol == 1)
    assert nbr is None or (nbr.dtype == torch.int32 and nbr.shape[0] == kvol and nbr.shape[1] >= n_out)
    if out is None:
        out = torch.empty((n_out, cout), dtype=torch.bfloat16, device=inp.device)
    assert tuple(out.shape) == (n_out, cout) and out.dtype == torch.bfloat16
    region = timed_begin()
    _check(lib().u3d_igemm_fwd_affine_bf16(_ptr(inp), _ptr(w_folded), _ptr(nbr), nbr.shape[1] if nbr is not None else 0, _ptr(shift),
                                           int(bool(relu)), _ptr(out), _ptr(n_out_dev), n_out, cin, cout, kvol, _stream()),
           "igemm_fwd_affine_bf16")
    if region is not None:
        timed_end(region, tag, inp.shape[0], n_out, cin, cout, kvol, nbr)
    return out


# --------------------------------------------------------------------------------------------------
# FP8 (OCP e4m3fn) inference of the wide dense convolutions (csrc/fp8.hip, csrc/igemm_fp8.hip).  Codes travel as uint8 tensors.
# --------------------------------------------------------------------------------------------------
FWD_FP8_KERNELS = tuple("fp8_glds8_" + n.lower() for n in _slot_names("U3D_FWD_FP8_K_"))      # 256x256, 192x256, 256x256_rows
FwdFp8Plan = collections.namedtuple("FwdFp8Plan", "kernel rows cols")


def fwd_fp8_plan(n_out, cin, cout, kvol, has_nbr):
    """The kernel and tile u3d_igemm_fwd_affine_fp8 takes for the shape, None when it does not serve it (cin % 128, cout % 128, kvol > 1
    with a table or kvol == 1 without one).  Host only: the library answers without a GPU."""
    k, r, c = C.c_int32(), C.c_int32(), C.c_int32()
    rc = lib().u3d_igemm_fwd_fp8_plan(n_out, cin, cout, kvol, bool(has_nbr), C.byref(k), C.byref(r), C.byref(c))
    if rc:
        return None if rc == U3D_ERR_UNSUPPORTED else _check(rc, "igemm_fwd_fp8_plan")
    return FwdFp8Plan(FWD_FP8_KERNELS[k.value], r.value, c.value)


def quant_rows_e4m3(x, e_dev, n_dev, out=None):
    """e4m3 codes (uint8 [n, C]) of the bf16 rows x under the power-of-two scale 2^e, e read from the device int32 e_dev: q(x, e) =
    e4m3_rne(clamp(x * 2^-e, -448, 448)).  Only the first *n_dev rows of `out` are written."""
    assert x.dtype == torch.bfloat16 and x.dim() == 2 and x.shape[1] % 8 == 0 and x.data_ptr() % 16 == 0
    assert e_dev.dtype == torch.int32 and e_dev.numel() == 1 and n_dev.dtype == torch.int32
    if out is None:
        out = torch.empty(tuple(x.shape), dtype=torch.uint8, device=x.device)
    assert tuple(out.shape) == tuple(x.shape) and out.dtype == torch.uint8 and out.data_ptr() % 8 == 0
    _check(lib().u3d_quant_rows_e4m3(_ptr(x), _ptr(out), _ptr(n_dev), x.shape[0], x.shape[1], _ptr(e_dev), _stream()), "quant_rows_e4m3")
    return out


def absmax_rows(x, n_dev, slot):
    """slot = max(slot, max |x|) over the first *n_dev rows of the bf16 rows x; slot: one f32 device element (a view of a per-layer
    table), zeroed by the caller.  Exact, order independent, no host sync; a NaN or Inf input leaves +Inf."""
    assert x.dtype == torch.bfloat16 and x.dim() == 2 and x.shape[1] % 8 == 0 and x.data_ptr() % 16 == 0
    assert slot.dtype == torch.float32 and slot.numel() == 1 and n_dev.dtype == torch.int32
    _check(lib().u3d_absmax_rows(_ptr(x), _ptr(n_dev), x.shape[0], x.shape[1], _ptr(slot), _stream()), "absmax_rows")
    return slot


BnFoldFp8Job = _struct("u3d_bn_fold_fp8_job", "BnFoldFp8Job")       # one record of u3d_bn_fold_fp8_batched's device job table


class BnFoldFp8Table(_FoldTable):
    """Folds AND quantises every pair.  destinations: qw uint8 [kvol, Cout, Cin], e_w int32 [Cout], shift f32 [Cout]."""
    ENTRY = "u3d_bn_fold_fp8_batched"

    def _jobs(self, pairs, geo):
        assert int(lib().u3d_bn_fold_fp8_job_bytes()) == C.sizeof(BnFoldFp8Job)
        jobs = (BnFoldFp8Job * len(pairs))()
        fb = 0
        for j, (w, layout, gamma, beta, mean, var, eps, qw, e_w, shift), (k, cout, cin, sk, sa, sb) in zip(jobs, pairs, geo):
            assert qw.is_cuda and qw.dtype == torch.uint8 and qw.is_contiguous() and tuple(qw.shape) == (k, cout, cin)
            assert e_w.is_cuda and e_w.dtype == torch.int32 and tuple(e_w.shape) == (cout,)
            assert shift.is_cuda and shift.dtype == torch.float32 and tuple(shift.shape) == (cout,)
            j.w, j.gamma, j.beta, j.mean, j.var = w.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), var.data_ptr()
            j.qw, j.e_w, j.shift = qw.data_ptr(), e_w.data_ptr(), shift.data_ptr()
            j.sk, j.sa, j.sb, j.eps = sk, sa, sb, float(eps)
            j.kvol, j.cout, j.cin, j.first_block = k, cout, cin, fb
            fb += cout
        return jobs, fb


def igemm_fwd_affine_fp8(qin, qw, nbr, colscale, shift, relu, n_out_dev, n_out, out=None, tag="spconv_fwd"):
    """out = act(conv(qin; qw) * colscale + shift) on the block-scaled fp8 MFMA (u3d_igemm_fwd_affine_fp8): qin uint8 [n_in, cin] and qw
    uint8 [kvol, cout, cin] e4m3 codes, nbr int32 [kvol, ld] or None for kvol == 1, colscale / shift f32 [cout], out bf16.  Rows at or
    past *n_out_dev of `out` are left as they are.  A shape fwd_fp8_plan does not serve is an error: there is no other route."""
    kvol, cout, cin = qw.shape
    assert qin.dtype == torch.uint8 and qw.dtype == torch.uint8 and shift.dtype == torch.float32 and colscale.dtype == torch.float32
    assert qin.shape[1] == cin and tuple(shift.shape) == (cout,) and tuple(colscale.shape) == (cout,) and (nbr is not None or kvol == 1)
    assert shift.data_ptr() % 16 == 0 and colscale.data_ptr() % 16 == 0
    assert nbr is None or (nbr.dtype == torch.int32 and nbr.shape[0] == kvol and nbr.shape[1] >= n_out)
    if out is None:
        out = torch.empty((n_out, cout), dtype=torch.bfloat16, device=qin.device)
    assert tuple(out.shape) == (n_out, cout) and out.dtype == torch.bfloat16
    region = timed_begin()
    _check(lib().u3d_igemm_fwd_affine_fp8(_ptr(qin), _ptr(qw), _ptr(nbr), nbr.shape[1] if nbr is not None else 0, _ptr(colscale),
                                          _ptr(shift), int(bool(relu)), _ptr(out), _ptr(n_out_dev), n_out, cin, cout, kvol, _stream()),
           "igemm_fwd_affine_fp8")
    if region is not None:
        timed_end(region, tag, qin.shape[0], n_out, cin, cout, kvol, nbr, in_bytes=1, w_bytes=1)      # e4m3 rows and weights in, bf16 rows out
    return out


def igemm_direct_affine(inp, w_folded, nbr, shift, relu, n_out_dev, n_out, addend=None, out=None, tag="spconv_fwd"):
    """act(conv(inp; w_folded) + shift + addend) on a narrow 27-offset level in one launch of the direct-operand kernel
    (u3d_igemm_direct_affine_bf16): inp bf16 [n_in, cin], w_folded bf16 [27, cout, cin] (bn_fold), nbr int32 [27, ld], shift f32 [cout],
    addend bf16 [n_out, cout] or None.  Rows at or past *n_out_dev of `out` are left as they are.  A shape direct_serves() does not
    name is an error: there is no other route."""
    kvol, cout, cin = w_folded.shape
    assert inp.dtype == torch.bfloat16 and w_folded.dtype == torch.bfloat16 and shift.dtype == torch.float32
    assert kvol == 27 and inp.shape[1] == cin and tuple(shift.shape) == (cout,) and shift.data_ptr() % 16 == 0
    assert nbr is not None and nbr.dtype == torch.int32 and nbr.shape[0] == kvol and nbr.shape[1] >= n_out
    assert addend is None or (addend.dtype == torch.bfloat16 and tuple(addend.shape) == (n_out, cout))
    if out is None:
        out = torch.empty((n_out, cout), dtype=torch.bfloat16, device=inp.device)
    assert tuple(out.shape) == (n_out, cout) and out.dtype == torch.bfloat16
    region = timed_begin()
    _check(lib().u3d_igemm_direct_affine_bf16(_ptr(inp), _ptr(w_folded), _ptr(nbr), nbr.shape[1], _ptr(shift), int(bool(relu)), _ptr(addend),
                                              _ptr(out), _ptr(n_out_dev), n_out, cin, cout, _stream()), "igemm_direct_affine_bf16")
    if region is not None:
        timed_end(region, tag, inp.shape[0], n_out, cin, cout, kvol, nbr)
    return out


def spconv_fwd_split(xs, w3, nbr3, n_out_dev, n_out, cout, want_stats=False, tag="spconv_fwd", addend=None):
    """Split-bf16 product (u3d_igemm_fwd_split_bf16): xs bf16 [2 * n_in, cin] planes, w3 bf16 [3K, cout, cin] = (wh, wl, wh), nbr3 int32
    [3K, ld] = (nbr, nbr, nbr + n_in) -> f32 [n_out, cout] (+ per-tile BatchNorm sums f64 [tiles, 2, cout], rows per tile)."""
    kvol3, cin = w3.shape[0], xs.shape[1]
    out = torch.empty((n_out, cout), dtype=torch.float32, device=xs.device)
    stats, tr = None, 0
    if want_stats:
        layout = fwd_stats_layout(n_out, cin, cout, kvol3, True)
        if layout is not None and layout[1]:
            stats = torch.empty((layout[0], 2, cout), dtype=torch.float64, device=xs.device)
            tr = layout[1]
    region = timed_begin()
    assert addend is None or (addend.dtype == torch.float32 and tuple(addend.shape) == (n_out, cout))
    _check(lib().u3d_igemm_fwd_split_bf16(_ptr(xs), _ptr(w3), _ptr(nbr3), nbr3.shape[1], _ptr(out), _ptr(n_out_dev), n_out, cin, cout, kvol3,
                                          _ptr(stats), _ptr(addend), _stream()), "igemm_fwd_split_bf16")
    if region is not None:
        timed_end(region, tag, xs.shape[0] // 2, n_out, cin, cout, kvol3 // 3, nbr3, split=True)      # (the first third of nbr3 is the plain table)
    return (out, stats, tr) if want_stats else out


WGRAD_KERNELS = ("none", "conv_in", "narrow", "glds8_256", "glds_256", "glds_128", "glds_64", "reg_32", "reg_16")


def igemm_wgrad_plan(n_out, cin, cout, kvol, has_nbr, out_oik=False, out_layout=None):
    """(kernel family, tile, nsplit, workspace bytes) u3d_igemm_wgrad_bf16 takes for the shape; None when it does not serve it.
    out_layout (0 / 1 / 2, see u3d_hip.h) overrides out_oik (= layout 1).  (u3d_igemm_wgrad_bf16_workspace answers only the bytes: the
    query of a binder that does not want the plan; this package does not call it.)"""
    k, tile, ns, ws = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int64(0)
    layout = (1 if out_oik else 0) if out_layout is None else int(out_layout)
    if lib().u3d_igemm_wgrad_plan(n_out, cin, cout, kvol, int(bool(has_nbr)), layout, C.byref(k), C.byref(tile), C.byref(ns),
                                  C.byref(ws)) != 0:
        return None
    return WGRAD_KERNELS[k.value], tile.value, ns.value, ws.value


def spconv_wgrad(inp, dout, nbr, n_out_dev, kvol, out_oik=False, out=None):
    """-> f32 [K, Cin, Cout]; with out_oik (bf16 second-generation path only): [Cout, Cin, K] (nn.Conv3d's layout).
    out: contiguous f32 tensor of kvol*cin*cout elements to write into (bf16 path) - returned viewed in the result's shape."""
    cin, cout, n_out = inp.shape[1], dout.shape[1], dout.shape[0]
    bf16 = bool(inp.dtype == torch.bfloat16 and USE_IGEMM_V2)
    v2 = bf16 and cin % 16 == 0 and cout % 16 == 0
    assert v2 or not out_oik, "out_oik needs the bf16 implicit-GEMM weight-gradient path"
    shape = (cout, cin, kvol) if out_oik else (kvol, cin, cout)
    # the implicit-GEMM plan decides (u3d_igemm_wgrad_plan): None = no second-generation kernel serves the shape (e.g. 32 -> 16 x 27,
    # channel counts off the 16 grid other than the 8 -> 16 input convolution) - the first-generation kernel then
    plan = igemm_wgrad_plan(n_out, cin, cout, kvol, nbr is not None, out_oik) if bf16 else None
    region = timed_begin()
    if plan is None and not v2:
        dw = spconv_wgrad_generic(inp, dout, nbr, n_out_dev, kvol)
    else:
        if out is not None and v2 and out.is_contiguous() and out.dtype == torch.float32 and out.numel() == kvol * cin * cout:
            dw = out.view(shape)
        else:
            dw = torch.empty(shape, dtype=torch.float32, device=inp.device)
        if plan is not None:
            ws = torch.empty(plan[3], dtype=torch.uint8, device=inp.device)
            _check(lib().u3d_igemm_wgrad_bf16(_ptr(inp), _ptr(dout), _ptr(nbr), nbr.shape[1] if nbr is not None else 0, _ptr(dw),
                                              _ptr(n_out_dev), n_out, cin, cout, kvol, 1 if out_oik else 0, _ptr(ws), plan[3], _stream()),
                   "igemm_wgrad_bf16")
        else:
            gen = spconv_wgrad_generic(inp, dout, nbr, n_out_dev, kvol)
            dw.copy_(gen.permute(2, 1, 0) if out_oik else gen)
    if region is not None:
        timed_end(region, "spconv_wgrad", inp.shape[0], n_out, cin, cout, kvol, nbr, act_bytes=inp.element_size(), w_bytes=4, v2=v2)
    return dw


def spconv_wgrad_active(dout, rows, t, n_dev, kvol, out=None):
    """Weight gradient of a convolution over a dense lattice whose input is zero off a sparse level's rows, summed over those rows
    only: dW[co][ci][k] = sum_{i < *n_dev} dout[t[k][i]][co] * rows[i][ci], f32 [Cout, Cin, K] (nn.Conv3d's layout).  dout bf16
    [n_out, Cout]; rows bf16 [cap, Cin], the level's features; t int32 [K, ld] from active_nbr_table (transposed tables).  The
    kernels of spconv_wgrad with the operands' roles exchanged (out_layout 2); no other kernel serves this: a missing plan is an error.
    out: as spconv_wgrad."""
    cap, cin = rows.shape
    cout = dout.shape[1]
    assert dout.dtype == torch.bfloat16 and rows.dtype == torch.bfloat16 and t.shape[0] == kvol and t.shape[1] >= cap
    plan = igemm_wgrad_plan(cap, cout, cin, kvol, True, out_layout=2)
    if plan is None:
        raise U3DError(f"no weight-gradient kernel serves {cin} -> {cout} x {kvol} over active rows")
    region = timed_begin()
    if out is not None and out.is_contiguous() and out.dtype == torch.float32 and out.numel() == kvol * cin * cout:
        dw = out.view(cout, cin, kvol)
    else:
        dw = torch.empty((cout, cin, kvol), dtype=torch.float32, device=rows.device)
    ws = torch.empty(plan[3], dtype=torch.uint8, device=rows.device)
    _check(lib().u3d_igemm_wgrad_bf16(_ptr(dout), _ptr(rows), _ptr(t), t.shape[1], _ptr(dw), _ptr(n_dev), cap, cout, cin, kvol, 2,
                                      _ptr(ws), plan[3], _stream()), "igemm_wgrad_bf16 (active rows)")
    if region is not None:
        timed_end(region, "spconv_wgrad", dout.shape[0], cap, cin, cout, kvol, t, act_bytes=2, w_bytes=4, v2=True)
    return dw


def spconv_wgrad_generic(inp, dout, nbr, n_out_dev, kvol):
    """First-generation weight gradient (any channel counts, f32 or bf16): f32 [K, Cin, Cout]."""
    cin, cout, n_out = inp.shape[1], dout.shape[1], dout.shape[0]
    dw = torch.empty((kvol, cin, cout), dtype=torch.float32, device=inp.device)
    wsb = int(lib().u3d_spconv_wgrad_workspace(n_out, cin, cout, kvol))
    ws = torch.empty(wsb, dtype=torch.uint8, device=inp.device)
    ld = nbr.shape[1] if nbr is not None else 0
    _check(lib().u3d_spconv_wgrad(_ptr(inp), _ptr(dout), _ptr(nbr), ld, _ptr(dw), _ptr(n_out_dev), n_out, cin, cout, kvol,
                                  dtype_code(inp), _ptr(ws), wsb, _stream()), "spconv_wgrad")
    return dw


def colsum(x):
    """f32 column sums of a dense [n, C] f32/bf16 matrix (fixed order; safe under HIP-graph replay, unlike torch's sum(0))."""
    x = x if x.is_contiguous() else x.contiguous()
    n, c = x.shape
    out = torch.empty((c,), dtype=torch.float32, device=x.device)
    wsb = int(lib().u3d_colsum_workspace(n, c))
    ws = torch.empty(max(wsb, 4), dtype=torch.uint8, device=x.device)
    _check(lib().u3d_colsum(_ptr(x), n, c, dtype_code(x), _ptr(out), _ptr(ws), wsb, _stream()), "colsum")
    return out


def bn_stats(x, n_dev):
    n, c = x.shape
    sums = torch.empty((2, c), dtype=torch.float64, device=x.device)
    wsb = int(lib().u3d_bn_stats_workspace(n, c))
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    _check(lib().u3d_bn_stats(_ptr(x), _ptr(n_dev), n, c, dtype_code(x), _ptr(sums), _ptr(ws), wsb, _stream()), "bn_stats")
    return sums


def bn_finalize(sums, n_dev, n_cap, eps, momentum, running_mean=None, running_var=None, num_batches=None):
    c = sums.shape[1]
    mean = torch.empty((c,), dtype=torch.float32, device=sums.device)
    invstd = torch.empty((c,), dtype=torch.float32, device=sums.device)
    _check(lib().u3d_bn_finalize(_ptr(sums), _ptr(n_dev), n_cap, c, eps, momentum, _ptr(running_mean), _ptr(running_var),
                                 _ptr(num_batches), _ptr(mean), _ptr(invstd), _stream()), "bn_finalize")
    return mean, invstd


def bn_forward_stats(x, n_dev, eps, momentum, running_mean=None, running_var=None, num_batches=None):
    """Training statistics of a row matrix: (mean, invstd) f32 [C]; updates the running statistics like nn.BatchNorm1d."""
    n, c = x.shape
    mean = torch.empty((c,), dtype=torch.float32, device=x.device)
    invstd = torch.empty((c,), dtype=torch.float32, device=x.device)
    wsb = int(lib().u3d_bn_stats_workspace(n, c))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=x.device)
    _check(lib().u3d_bn_forward_stats(_ptr(x), _ptr(n_dev), n, c, dtype_code(x), eps, momentum, _ptr(running_mean), _ptr(running_var),
                                      _ptr(num_batches), _ptr(mean), _ptr(invstd), _ptr(ws), ws.numel(), _stream()), "bn_forward_stats")
    return mean, invstd


def bn_apply(x, mean, invstd, gamma, beta, residual, relu, n_dev, row_map=None, post_add=None, want_planes=False):
    """row_map (int32 [n], a bijection): row r of x lands in row row_map[r] of y (see include/u3d_hip.h).
    want_planes (f32 rows): -> (y, planes) with planes bf16 [2 * n, c] = split_rows(y) written by the same pass, or (y, None) for a
    shape the fused pass does not take."""
    n, c = x.shape
    y = torch.empty_like(x)
    planes = torch.empty((2 * n, c), dtype=torch.bfloat16, device=x.device) if want_planes and x.dtype == torch.float32 else None
    for planes in (planes, None):       # one retry without the planes when the fused pass does not take the shape
        rc = lib().u3d_bn_apply(_ptr(x), _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(beta), _ptr(residual), int(relu), _ptr(y), _ptr(planes),
                                _ptr(n_dev), n, c, dtype_code(x), _ptr(row_map), _ptr(post_add), _stream())
        if planes is None or rc != U3D_ERR_UNSUPPORTED:
            break
    _check(rc, "bn_apply")
    return (y, planes) if want_planes else y


def bn_bwd_stats(dy, y, x, mean, invstd, relu, n_dev, gamma=None, beta=None, row_map=None, want_f32=False):
    """y may be None (relu, no residual in the forward): the ReLU mask is recomputed from x with gamma/beta."""
    n, c = x.shape
    sums = torch.empty((2, c), dtype=torch.float64, device=x.device)
    wsb = int(lib().u3d_bn_stats_workspace(n, c))
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    s32 = torch.empty((2, c), dtype=torch.float32, device=x.device) if want_f32 else None
    _check(lib().u3d_bn_bwd_stats(_ptr(dy), _ptr(y), _ptr(x), _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(beta), int(relu), _ptr(n_dev), n, c,
                                  dtype_code(x), _ptr(sums), _ptr(ws), wsb, _ptr(row_map), _ptr(s32), _stream()), "bn_bwd_stats")
    return (sums, s32) if want_f32 else sums


def bn_bwd_apply(dy, y, x, mean, invstd, gamma, sums, relu, n_dev, want_dres, beta=None, row_map=None, want_planes=False):
    """want_planes (f32 rows): -> (dx, dres, planes of dx or None)."""
    n, c = x.shape
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_dres else None
    planes = torch.empty((2 * n, c), dtype=torch.bfloat16, device=x.device) if want_planes and x.dtype == torch.float32 else None
    for planes in (planes, None):       # as bn_apply
        rc = lib().u3d_bn_bwd_apply(_ptr(dy), _ptr(y), _ptr(x), _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(beta), _ptr(sums), int(relu),
                                    _ptr(dx), _ptr(dres), _ptr(planes), _ptr(n_dev), n, c, dtype_code(x), _ptr(row_map), _stream())
        if planes is None or rc != U3D_ERR_UNSUPPORTED:
            break
    _check(rc, "bn_bwd_apply")
    return (dx, dres, planes) if want_planes else (dx, dres)


def _opt_ptr_array(tensors):
    """_ptr_array with None entries (NULL)."""
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        assert t is None or (t.is_cuda and t.is_contiguous()), "device-contiguous tensor required"
        arr[i] = None if t is None else t.data_ptr()
    return arr


def bn_apply_sum(xs, means, invstds, gammas, betas, idxs, n_dev):
    """out = sum_i relu(bn_i(xs[i][idxs[i]])) in one launch (u3d_bn_apply_sum; idxs[i] int32 [n] or None), every partial sum rounded to
    bf16 as the chain of bn_apply(..., post_add) calls rounds it.  -> None for what the kernel does not take (the caller runs the chain)."""
    n, c = xs[0].shape
    assert all(x.shape == (n, c) and x.dtype == xs[0].dtype for x in xs)
    out = torch.empty_like(xs[0])
    rc = lib().u3d_bn_apply_sum(_opt_ptr_array(xs), _opt_ptr_array(means), _opt_ptr_array(invstds), _opt_ptr_array(gammas),
                                _opt_ptr_array(betas), _opt_ptr_array(idxs), len(xs), _ptr(out), _ptr(n_dev), n, c, dtype_code(xs[0]),
                                _stream())
    if rc == U3D_ERR_UNSUPPORTED:
        return None
    _check(rc, "bn_apply_sum")
    return out


def bn_bwd_apply_sum(dout, xs, means, invstds, gammas, betas, sums, idxs, n_dev):
    """The dx_i of bn_apply_sum's levels from one read of dout (u3d_bn_bwd_apply_sum); sums[i]: that level's bn_bwd_stats."""
    n, c = dout.shape
    dxs = [torch.empty_like(x) for x in xs]
    _check(lib().u3d_bn_bwd_apply_sum(_ptr(dout), _opt_ptr_array(xs), _opt_ptr_array(means), _opt_ptr_array(invstds),
                                      _opt_ptr_array(gammas), _opt_ptr_array(betas), _opt_ptr_array(sums), _opt_ptr_array(idxs),
                                      _opt_ptr_array(dxs), len(xs), _ptr(n_dev), n, c, dtype_code(dout), _stream()), "bn_bwd_apply_sum")
    return dxs


def to_dense(feat, coors, n_dev, batch, dims):
    """-> logical [B, C, D, H, W] tensor in channels_last_3d memory format."""
    n, c = feat.shape
    dz, dy, dx = dims
    vol = torch.zeros((batch, dz, dy, dx, c), dtype=feat.dtype, device=feat.device)
    _check(lib().u3d_to_dense(_ptr(feat), _ptr(coors), _ptr(n_dev), n, c, _ptr(vol), dz, dy, dx, dtype_code(feat), _stream()),
           "to_dense")
    return vol.permute(0, 4, 1, 2, 3)


def from_dense(vol_cl, coors, n_dev, n):
    """vol_cl: contiguous [B, Dz, Dy, Dx, C] -> rows [n, C]."""
    b, dz, dy, dx, c = vol_cl.shape
    feat = torch.empty((n, c), dtype=vol_cl.dtype, device=vol_cl.device)
    _check(lib().u3d_from_dense(_ptr(vol_cl), _ptr(coors), _ptr(n_dev), n, c, _ptr(feat), dz, dy, dx, dtype_code(vol_cl),
                                _stream()), "from_dense")
    return feat


def gather_rows(inp, idx):
    n = idx.shape[0]
    out = torch.empty((n,) + tuple(inp.shape[1:]), dtype=inp.dtype, device=inp.device)
    row_bytes = inp[0].numel() * inp.element_size()
    _check(lib().u3d_gather_rows(_ptr(inp), _ptr(idx), n, row_bytes, _ptr(out), _stream()), "gather_rows")
    return out


def scatter_rows(inp, idx, n_out):
    out = torch.zeros((n_out,) + tuple(inp.shape[1:]), dtype=inp.dtype, device=inp.device)
    row_bytes = inp[0].numel() * inp.element_size()
    _check(lib().u3d_scatter_rows(_ptr(inp), _ptr(idx), idx.shape[0], row_bytes, _ptr(out), _stream()), "scatter_rows")
    return out


# --------------------------------------------------------------------------------------------------
# query side: FPS, matching, IoU
# --------------------------------------------------------------------------------------------------
FPS_REG_MAX = 20480


def fps_err_buffer(device):
    """int32 [2] time-out record of FPS calls over sets above FPS_REG_MAX points (include/u3d_hip.h u3d_fps): [0] = this call timed
    out (its samples must not be used), [1] = calls that timed out so far.  Owned by the caller (TrainStep keeps one and feeds [0]
    into the step's collective hold flag); reading it synchronises with the device."""
    return torch.zeros(2, dtype=torch.int32, device=device)


def _fps_err_arg(err, max_n, device):
    """The several-workgroup form REQUIRES the record; smaller sets never write it (and a captured step saves the clearing launch)."""
    if max_n <= FPS_REG_MAX:
        return None
    return fps_err_buffer(device) if err is None else err


def fps(base, set_off, set_n, max_n, m, err=None, poll_ticks=0, max_wg=0):
    """base: f32 device buffer; set_off int64 [S] element offsets; set_n int32 [S]; -> idx int32 [S, m].
    err: int32 [2] from fps_err_buffer() (None: a private one, reachable as `idx._u3d_fps_err`); poll_ticks / max_wg: the C ABI's
    time-out limit (100 MHz ticks, 0 = 0.5 s) and resident-workgroup budget (0 = 3/4 of the device's CUs, 1 = streaming kernel)."""
    nsets = set_off.shape[0]
    out = torch.empty((nsets, m), dtype=torch.int32, device=base.device)
    temp, stride = None, 0
    if max_n > FPS_REG_MAX:
        temp = torch.empty((nsets, max_n), dtype=torch.float32, device=base.device)
        stride = max_n
    err = _fps_err_arg(err, max_n, base.device)
    _check(lib().u3d_fps(_ptr(base), _ptr(set_off), _ptr(set_n), nsets, max_n, m, _ptr(out), _ptr(temp), stride, _ptr(err), int(poll_ticks),
                         int(max_wg), _stream()), "fps")
    out._u3d_fps_err = err
    return out


def fps_queries(points, coors, scene_off, voxel_off, batch, max_n, m, err=None, poll_ticks=0, max_wg=0):
    """The detector's two FPS passes + their glue in three launches (u3d_fps_prep | u3d_fps2 | u3d_fps_points).
    points f32 [N,F] (packed-triple view: the reference hands the whole [N,F] buffer to the sampler), coors int32 [V,4] (b,z,y,x),
    scene_off / voxel_off int32 [B+1] -> fpsbpts f32 [B, 2m, 3] in the unit cube (ref: uni3detr.py:178-189).  err / poll_ticks /
    max_wg: as fps()."""
    dev = points.device
    F_ = points.shape[1]
    V = coors.shape[0]
    vox = torch.empty((max(V, 1), 3), dtype=torch.float32, device=dev)
    set_off = torch.empty((2 * batch,), dtype=torch.int64, device=dev)
    set_n = torch.empty((2 * batch,), dtype=torch.int32, device=dev)
    _check(lib().u3d_fps_prep(_ptr(coors), V, _ptr(scene_off), _ptr(voxel_off), batch, F_, _ptr(vox), _ptr(set_off), _ptr(set_n), _stream()),
           "fps_prep")
    idx = torch.empty((2 * batch, m), dtype=torch.int32, device=dev)
    temp, stride = None, 0
    if max_n > FPS_REG_MAX:
        temp = torch.empty((2 * batch, max_n), dtype=torch.float32, device=dev)
        stride = max_n
    err = _fps_err_arg(err, max_n, dev)
    _check(lib().u3d_fps2(_ptr(points), _ptr(vox), batch, _ptr(set_off), _ptr(set_n), 2 * batch, max_n, m, _ptr(idx), _ptr(temp), stride,
                          _ptr(err), int(poll_ticks), int(max_wg), _stream()), "fps2")
    idx._u3d_fps_err = err
    out = torch.empty((batch, 2 * m, 3), dtype=torch.float32, device=dev)
    _check(lib().u3d_fps_points(_ptr(points), F_, _ptr(vox), _ptr(idx), _ptr(scene_off), _ptr(voxel_off), batch, m, _ptr(out), _stream()),
           "fps_points")
    return out, idx


def loss_targets(asg, gt, labels, gt_off, ncls):
    """asg int32 [L,B,Q], gt f32 [sumG,gd], labels int32 [sumG] -> (asg int64, w f32 [L,B,Q], tgt f32 [L,B,Q,gd], lab int64, num_pos f32 [L])."""
    L, B, Q = asg.shape
    gd = gt.shape[1]
    dev = asg.device
    a64 = torch.empty((L, B, Q), dtype=torch.int64, device=dev)
    w = torch.empty((L, B, Q), dtype=torch.float32, device=dev)
    tgt = torch.empty((L, B, Q, gd), dtype=torch.float32, device=dev)
    lab = torch.empty((L, B, Q), dtype=torch.int64, device=dev)
    npos = torch.empty((L,), dtype=torch.float32, device=dev)
    _check(lib().u3d_loss_targets(_ptr(asg), _ptr(gt), _ptr(labels), _ptr(gt_off), L, B, Q, gd, ncls, _ptr(a64), _ptr(w), _ptr(tgt), _ptr(lab),
                                  _ptr(npos), _stream()), "loss_targets")
    return a64, w, tgt, lab, npos


def query_embed_fwd(tgt, anchor, fps, rnd, groups):
    """-> (query_embeds [B,G*nq,c+3], query [B,G*nq,c], ref_logits [B,G*nq,3], sigmoid(ref_logits)) f32 (u3d_query_embed_fwd)."""
    B, nq, c = fps.shape[0], anchor.shape[0], tgt.shape[1]
    dev = tgt.device
    qe = torch.empty((B, groups * nq, c + 3), dtype=torch.float32, device=dev)
    q = torch.empty((B, groups * nq, c), dtype=torch.float32, device=dev)
    r = torch.empty((B, groups * nq, 3), dtype=torch.float32, device=dev)
    rs = torch.empty((B, groups * nq, 3), dtype=torch.float32, device=dev)
    _check(lib().u3d_query_embed_fwd(_ptr(tgt), _ptr(anchor), _ptr(fps), _ptr(rnd), B, nq, groups, c, _ptr(qe), _ptr(q), _ptr(r), _ptr(rs),
                                     _stream()), "query_embed_fwd")
    return qe, q, r, rs


def query_embed_bwd(dqe, dq, dr, drs, anchor, B, nq, groups, c, device):
    dt = torch.empty((2 * nq, c), dtype=torch.float32, device=device)
    da = torch.empty((nq, 3), dtype=torch.float32, device=device)
    _check(lib().u3d_query_embed_bwd(_ptr(dqe), _ptr(dq), _ptr(dr), _ptr(drs), _ptr(anchor), B, nq, groups, c, _ptr(dt), _ptr(da), _stream()),
           "query_embed_bwd")
    return dt, da


def match_cost(cls, box, gt, labels, gt_off, gmax, w_cls, w_reg, w_iou, alpha=0.25, gamma=2.0):
    """cls [L,B,Q,C], box [L,B,Q,code] f32; gt [sumG,7] gravity-centre; labels int32; -> cost f32 [L*B, gmax, Q]."""
    L, B, Q, Ccls = cls.shape
    cost = torch.zeros((L * B, gmax, Q), dtype=torch.float32, device=cls.device)
    _check(lib().u3d_match_cost(_ptr(cls), _ptr(box), _ptr(gt), _ptr(labels), _ptr(gt_off), L, B, Q, Ccls, box.shape[-1], gmax,
                                w_cls, w_reg, w_iou, alpha, gamma, _ptr(cost), _stream()), "match_cost")
    return cost


def lsa(cost, gt_off, L, B, Q, nq, gmax):
    assigned = torch.empty((L, B, Q), dtype=torch.int32, device=cost.device)
    _check(lib().u3d_lsa(_ptr(cost), _ptr(gt_off), L, B, Q, nq, gmax, _ptr(assigned), _stream()), "lsa")
    return assigned


def iou3d_rotated_aligned(a, b):
    n = a.shape[0]
    out = torch.empty((n,), dtype=torch.float32, device=a.device)
    _check(lib().u3d_iou3d_rotated_aligned(_ptr(a), _ptr(b), n, _ptr(out), _stream()), "iou3d_rotated_aligned")
    return out


def trilinear_fwd(value_rows, grid, batch, dims):
    """value_rows [B*D*H*W, C] contiguous; grid f32 [B,N,3] -> [B,N,C]."""
    nq, c = grid.shape[1], value_rows.shape[1]
    out = torch.empty((batch, nq, c), dtype=value_rows.dtype, device=value_rows.device)
    _check(lib().u3d_trilinear_fwd(_ptr(value_rows), _ptr(grid), batch, nq, dims[0], dims[1], dims[2], c, _ptr(out),
                                   dtype_code(value_rows), _stream()), "trilinear_fwd")
    return out


def trilinear_bwd(value_rows, grid, dout, batch, dims, want_dvalue=True, want_dgrid=True, dvalue_accum=None):
    """dvalue_accum: an existing f32 [rows, C] buffer to ACCUMULATE the value gradient into (the kernel adds with atomics)."""
    nq, c = grid.shape[1], value_rows.shape[1]
    if want_dvalue:
        dvalue = dvalue_accum if dvalue_accum is not None else torch.zeros(value_rows.shape, dtype=torch.float32, device=value_rows.device)
    else:
        dvalue = None
    dgrid = torch.empty((batch, nq, 3), dtype=torch.float32, device=value_rows.device) if want_dgrid else None
    _check(lib().u3d_trilinear_bwd(_ptr(value_rows), _ptr(grid), _ptr(dout), batch, nq, dims[0], dims[1], dims[2], c, _ptr(dvalue),
                                   _ptr(dgrid), dtype_code(value_rows), _stream()), "trilinear_bwd")
    return dvalue, dgrid


def nms3d_classwise(boxes, scores, labels, thr):
    """boxes [n,7], scores [n], labels [n] -> indices kept, ordered by (label asc, score desc) like the reference's
    per-class loop over mmcv.ops.nms3d."""
    n = boxes.shape[0]
    if n == 0:
        return torch.zeros((0,), dtype=torch.long, device=boxes.device)
    order = torch.argsort(scores, descending=True, stable=True)
    b = boxes[order, :7].float().contiguous()
    l = labels[order].int().contiguous()
    keep = torch.empty((n,), dtype=torch.uint8, device=boxes.device)
    wsb = int(lib().u3d_nms3d_workspace(n))
    ws = torch.empty(wsb, dtype=torch.uint8, device=boxes.device)
    _check(lib().u3d_nms3d(_ptr(b), _ptr(l), n, float(thr), _ptr(keep), _ptr(ws), wsb, _stream()), "nms3d")
    kept = order[keep.bool()]
    return kept[torch.argsort(labels[kept], stable=True)]


_COUNT_CACHE = {}


def soft_nms_classwise(boxes, scores, labels, num_classes, sigma, prune):
    """-> (idx long [k] into the input, decayed scores [k], labels long [k]) class-major, selection order inside a class."""
    n = boxes.shape[0]
    dev = boxes.device
    if n == 0:
        return (torch.zeros(0, dtype=torch.long, device=dev), torch.zeros(0, device=dev), torch.zeros(0, dtype=torch.long, device=dev))
    b = boxes[:, :7].contiguous().float()
    oi = torch.empty((num_classes, n), dtype=torch.int32, device=dev)
    os_ = torch.empty((num_classes, n), dtype=torch.float32, device=dev)
    oc = torch.empty((num_classes,), dtype=torch.int32, device=dev)
    _check(lib().u3d_soft_nms(_ptr(b), _ptr(scores.contiguous().float()), _ptr(labels.contiguous().int()), n, num_classes, float(sigma),
                              float(prune), _ptr(oi), _ptr(os_), _ptr(oc), _stream()), "soft_nms")
    sel = torch.arange(n, device=dev)[None, :] < oc[:, None]              # variable-size result: the one sync of this routine
    cls = torch.arange(num_classes, device=dev)[:, None].expand(-1, n)
    return oi[sel].long(), os_[sel], cls[sel]


def box_merge(boxes_sorted, labels_sorted, thr):
    """boxes f32 [n,7] sorted by descending score -> (merged [n,7], keep bool [n])."""
    n = boxes_sorted.shape[0]
    dev = boxes_sorted.device
    merged = torch.empty((n, 7), dtype=torch.float32, device=dev)
    keep = torch.zeros((n,), dtype=torch.uint8, device=dev)
    if n == 0:
        return merged, keep.bool()
    ws = torch.empty(max(int(lib().u3d_box_merge_workspace(n)), 16), dtype=torch.uint8, device=dev)
    # named locals: the copy of a column slice must stay alive until the launch, or the allocator hands its block to the labels' copy
    b, l = boxes_sorted.contiguous().float(), labels_sorted.contiguous().int()
    _check(lib().u3d_box_merge(_ptr(b), _ptr(l), n, float(thr), _ptr(merged), _ptr(keep), _ptr(ws), ws.numel(), _stream()), "box_merge")
    return merged, keep.bool()


def eval_iou_argmax(det_boxes, det_scores, det_labels, det_off, gt_boxes, gt_labels, gt_off):
    """Per detection: best same-scene, same-class GT -> (iou_max f32 [N] (-inf: none), jmax int32 [N] (-1: none), sort key int64 [N])."""
    n, dev = det_boxes.shape[0], det_off.device
    iou = torch.empty((n,), dtype=torch.float32, device=dev)
    jmax = torch.empty((n,), dtype=torch.int32, device=dev)
    key = torch.empty((n,), dtype=torch.int64, device=dev)
    _check(lib().u3d_eval_iou_argmax(_ptr(det_boxes), _ptr(det_scores), _ptr(det_labels), _ptr(det_off), _ptr(gt_boxes), _ptr(gt_labels),
                                     _ptr(gt_off), det_off.numel() - 1, n, _ptr(iou), _ptr(jmax), _ptr(key), _stream()), "eval_iou_argmax")
    return iou, jmax, key


def eval_indoor(det_boxes, det_scores, det_labels, det_off, gt_boxes, gt_labels, gt_off, num_classes, thr):
    """Indoor AP / recall on the device (u3d_eval_*).  Boxes f32 [.,7] bottom-centre, labels int32, offsets int32 [S+1], thr f32 [T]
    (device).  -> dict of device tensors: iou_max, jmax, perm (rank -> detection), seg [C,2], npos [C], tp uint8 [T,N] (rank order),
    ap f32 [T,C], rec f64 [T,C].  No host synchronisation."""
    n, g, t = det_boxes.shape[0], gt_boxes.shape[0], thr.numel()
    dev = det_off.device
    iou, jmax, key = eval_iou_argmax(det_boxes, det_scores, det_labels, det_off, gt_boxes, gt_labels, gt_off)
    key_s, perm = torch.sort(key, stable=True)                 # stable: ties keep (scene, position in the scene)
    seg = torch.empty((num_classes, 2), dtype=torch.int32, device=dev)
    npos = torch.empty((num_classes,), dtype=torch.int32, device=dev)
    _check(lib().u3d_eval_segments(_ptr(key_s), n, _ptr(gt_labels), g, num_classes, _ptr(seg), _ptr(npos), _stream()), "eval_segments")
    first = torch.empty((t, g), dtype=torch.int32, device=dev)
    tp = torch.empty((t, n), dtype=torch.uint8, device=dev)
    _check(lib().u3d_eval_first_hit(_ptr(perm), n, _ptr(iou), _ptr(jmax), _ptr(thr), t, g, _ptr(first), _stream()), "eval_first_hit")
    _check(lib().u3d_eval_tp(_ptr(perm), n, _ptr(iou), _ptr(jmax), _ptr(thr), t, g, _ptr(first), _ptr(tp), _stream()), "eval_tp")
    prec = torch.empty((t, g), dtype=torch.float64, device=dev)
    ap = torch.empty((t, num_classes), dtype=torch.float32, device=dev)
    rec = torch.empty((t, num_classes), dtype=torch.float64, device=dev)
    _check(lib().u3d_eval_ap(_ptr(tp), n, _ptr(seg), _ptr(npos), num_classes, t, g, _ptr(prec), _ptr(ap), _ptr(rec), _stream()), "eval_ap")
    return dict(iou_max=iou, jmax=jmax, perm=perm, seg=seg, npos=npos, tp=tp, ap=ap, rec=rec)


KITTI_NT = 41


def compact_rows(rec, valid, off):
    """The rows of rec [n, k] with valid int32 [n] set, in input order (u3d_compact_rows after an ATen scan of the flags), and the
    offsets int32 [S+1] of the kept rows for the CSR offsets `off` of the input.  -> (out [m, k], new_off).  One host synchronisation (m)."""
    dev = off.device
    incl = torch.cat([torch.zeros(1, dtype=torch.int32, device=dev), torch.cumsum(valid, 0, dtype=torch.int32)])
    new_off = incl[off.long()].to(torch.int32).contiguous()
    pos = incl[:-1].contiguous()
    m = int(incl[-1])
    out = torch.empty((m, rec.shape[1]), dtype=rec.dtype, device=dev)
    if m:                                                                    # nothing kept: nothing to launch (and `out` has no storage)
        _check(lib().u3d_compact_rows(_ptr(rec), _ptr(valid), _ptr(pos), rec.shape[0], rec.shape[1] * rec.element_size(), _ptr(out),
                                      _stream()), "compact_rows")
    return out, new_off


def kitti_convert(boxes, scores, labels, off, calib, img, label_code, lim):
    """LiDAR detections -> KITTI records (u3d_kitti_convert + a stable compaction).  boxes f32 [n,7] bottom-centre, scores f32 [n],
    labels int32 [n], off int32 [S+1], calib f32 [S,32], img f32 [S,2] (H, W), label_code int32 [L], lim f32 [6] (all on the device).
    -> (records f32 [m,16] of the valid detections in input order, their offsets int32 [S+1]).  One host synchronisation (m)."""
    n, S = boxes.shape[0], off.numel() - 1
    dev = off.device
    rec = torch.empty((n, 16), dtype=torch.float32, device=dev)
    valid = torch.empty((n,), dtype=torch.int32, device=dev)
    _check(lib().u3d_kitti_convert(_ptr(boxes), _ptr(scores), _ptr(labels), _ptr(off), S, n, _ptr(calib), _ptr(img), _ptr(label_code),
                                   label_code.numel(), _ptr(lim), _ptr(rec), _ptr(valid), _stream()), "kitti_convert")
    return compact_rows(rec, valid, off)


def kitti_eval_core(dt, dt_off, gt, gt_off, cls, gfid, gmet, gmin, aos, dt_counts, gt_counts):
    """KITTI AP on the device (u3d_kitti_*).  dt / gt: records f32 [.,16], offsets int32 [S+1], cls int32 [K] class codes, groups gfid /
    gmet int32 [NG], gmin f32 [NG] (device); dt_counts / gt_counts: the per-scene counts as host lists (buffer sizes, LDS size).
    -> dict of device tensors: ov f32 [3,P], ov_off, gt_flag / dt_flag int8 [3K,.], nvalid [3K], dc_iof, tp_sc [NG,G] (sorted
    descending), thr [NG,41], nthr [NG], tot int32 [NG,3,41], sim f64 [NG,41], ap f64 [NG,4]."""
    dev = dt_off.device
    S, N, G, K, NG = len(dt_counts), dt.shape[0], gt.shape[0], cls.numel(), gfid.numel()
    pairs = [int(a) * int(b) for a, b in zip(dt_counts, gt_counts)]
    ov_off_h = [0]
    for p in pairs:
        ov_off_h.append(ov_off_h[-1] + p)
    P = ov_off_h[-1]
    ov_off = torch.tensor(ov_off_h, dtype=torch.int64, device=dev)
    ov = torch.empty((3, P), dtype=torch.float32, device=dev)
    _check(lib().u3d_kitti_overlaps(_ptr(dt), _ptr(dt_off), _ptr(gt), _ptr(gt_off), _ptr(ov_off), S, P, _ptr(ov), _stream()), "kitti_overlaps")
    gt_flag = torch.empty((3 * K, G), dtype=torch.int8, device=dev)
    dt_flag = torch.empty((3 * K, N), dtype=torch.int8, device=dev)
    nvalid = torch.empty((3 * K,), dtype=torch.int32, device=dev)
    dc_iof = torch.empty((N,), dtype=torch.float32, device=dev)
    _check(lib().u3d_kitti_flags(_ptr(dt), _ptr(dt_off), S, N, _ptr(gt), _ptr(gt_off), G, _ptr(cls), K, _ptr(gt_flag), _ptr(nvalid),
                                 _ptr(dt_flag), _ptr(dc_iof), _stream()), "kitti_flags")
    tp_sc = torch.empty((NG, G), dtype=torch.float32, device=dev)
    max_dt = max([int(c) for c in dt_counts] + [0])
    _check(lib().u3d_kitti_pass1(_ptr(dt), _ptr(dt_off), N, _ptr(gt_off), G, S, _ptr(ov_off), P, _ptr(ov), _ptr(gt_flag), _ptr(dt_flag),
                                 _ptr(gfid), _ptr(gmet), _ptr(gmin), NG, max_dt, _ptr(tp_sc), _stream()), "kitti_pass1")
    tp_sc = torch.sort(tp_sc, dim=1, descending=True).values.contiguous()      # only the values matter
    thr = torch.zeros((NG, KITTI_NT), dtype=torch.float32, device=dev)
    nthr = torch.empty((NG,), dtype=torch.int32, device=dev)
    _check(lib().u3d_kitti_thresholds(_ptr(tp_sc), G, NG, _ptr(gfid), _ptr(nvalid), _ptr(thr), _ptr(nthr), _stream()), "kitti_thresholds")
    lds = max([int(lib().u3d_kitti_pass2_lds(int(a), int(b))) for a, b in zip(dt_counts, gt_counts)] + [0])
    st = [torch.empty((NG, S, KITTI_NT), dtype=torch.int32, device=dev) for _ in range(3)]
    st_sim = torch.empty((NG, S, KITTI_NT), dtype=torch.float64, device=dev)
    _check(lib().u3d_kitti_pass2(_ptr(dt), _ptr(dt_off), N, _ptr(gt), _ptr(gt_off), G, S, _ptr(ov_off), P, _ptr(ov), _ptr(gt_flag),
                                 _ptr(dt_flag), _ptr(dc_iof), _ptr(gfid), _ptr(gmet), _ptr(gmin), _ptr(thr), _ptr(nthr), NG, int(aos), lds,
                                 _ptr(st[0]), _ptr(st[1]), _ptr(st[2]), _ptr(st_sim), _stream()), "kitti_pass2")
    tot = torch.empty((NG, 3, KITTI_NT), dtype=torch.int32, device=dev)
    sim = torch.empty((NG, KITTI_NT), dtype=torch.float64, device=dev)
    ap = torch.empty((NG, 4), dtype=torch.float64, device=dev)
    _check(lib().u3d_kitti_reduce(_ptr(st[0]), _ptr(st[1]), _ptr(st[2]), _ptr(st_sim), S, _ptr(nthr), NG, _ptr(tot), _ptr(sim), _ptr(ap),
                                  _stream()), "kitti_reduce")
    return dict(ov=ov, ov_off=ov_off, gt_flag=gt_flag, dt_flag=dt_flag, nvalid=nvalid, dc_iof=dc_iof, tp_sc=tp_sc, thr=thr, nthr=nthr,
                tot=tot, sim=sim, ap=ap)


NUSC_REC, NUSC_NTH, NUSC_NI = 12, 4, 101


def nusc_to_global(rows, cls, attr, aux, off, calib, is_pred, cls_range, attr_moving, attr_still, bike, gt_rec=None, gt_off=None):
    """nuScenes boxes -> filtered global records (u3d_nusc_convert, u3d_nusc_filter + a stable compaction).  rows f64 [n,9] LiDAR
    (x, y, z, l, w, h, yaw, vx, vy), cls int32 [n], attr int32 [n] (GT; None for predictions), aux f64 [n] (score / points), off int32
    [S+1], calib f64 [S,24], cls_range f64 [C], attr_moving / attr_still / bike int32 [C]; gt_rec / gt_off: the converted, uncompacted GT
    of the same samples (its rack rows) for predictions, None for GT itself.
    -> (all f64 [n,12] before the filters, valid int32 [n], records f64 [m,12] of the valid rows in input order, offsets int32 [S+1]).
    One host synchronisation (m)."""
    n, S, C = rows.shape[0], off.numel() - 1, cls_range.numel()
    dev = off.device
    rec = torch.empty((n, NUSC_REC), dtype=torch.float64, device=dev)
    valid = torch.empty((n,), dtype=torch.int32, device=dev)
    _check(lib().u3d_nusc_convert(_ptr(rows), _ptr(cls), _ptr(attr), _ptr(aux), _ptr(off), S, n, _ptr(calib), int(is_pred), _ptr(cls_range),
                                  _ptr(attr_moving), _ptr(attr_still), C, _ptr(rec), _ptr(valid), _stream()), "nusc_convert")
    if gt_rec is None:
        gt_rec, gt_off = rec, off
    _check(lib().u3d_nusc_filter(_ptr(rec), _ptr(off), S, n, int(is_pred), _ptr(calib), _ptr(gt_rec) if gt_rec.numel() else None,
                                 _ptr(gt_off), _ptr(cls_range), _ptr(bike), C, _ptr(valid), _stream()), "nusc_filter")
    out, new_off = compact_rows(rec, valid, off)
    return rec, valid, out, new_off


def _segments(key, n_seg):
    """stable order of int64 keys in [0, n_seg) and their CSR offsets int32 [n_seg+1]"""
    order = torch.sort(key, stable=True).indices
    seg = torch.zeros(n_seg + 1, dtype=torch.int64, device=key.device)
    seg[1:] = torch.cumsum(torch.bincount(key, minlength=n_seg), 0)
    return order, seg.to(torch.int32)


def nusc_metrics(pred, pred_off, gt, gt_off, n_cls, ths, tp_th, rec_interp, period):
    """nuScenes matching and accumulation over filtered global records (u3d_nusc_rank_keys, u3d_nusc_match, u3d_nusc_accumulate; ATen
    sorts the keys).  pred / gt f64 [.,12] with offsets int32 [S+1], ths f64 [4], rec_interp f64 [101], period f64 [C] (device).
    -> dict of device tensors: rank int32 [n] (prediction rows in rank order), cseg int32 [C+1], npos int32 [C], tp int8 [4,n] and
    match int32 [n] by rank position, prec / conf f64 [C,4,101], err f64 [C,5,101], ap f64 [C,4], tp_err f64 [C,5], mri int32 [C,4].
    One host synchronisation (the largest GT segment, for the LDS size)."""
    dev = pred_off.device
    n, g, S, C = pred.shape[0], gt.shape[0], pred_off.numel() - 1, n_cls
    samp = lambda off, m: torch.repeat_interleave(torch.arange(S, device=dev), (off[1:] - off[:-1]).long(), output_size=m)  # noqa: E731
    key = torch.empty((n,), dtype=torch.int64, device=dev)
    idx = torch.empty((n,), dtype=torch.int32, device=dev)
    _check(lib().u3d_nusc_rank_keys(_ptr(pred), n, _ptr(key), _ptr(idx), _stream()), "nusc_rank_keys")
    by_score = idx.long()[torch.sort(key, stable=True).indices]              # (score desc, row desc)
    pcls = pred[:, 10].long()
    o, cseg = _segments(pcls[by_score], C)
    rank = by_score[o]
    mkey = pcls[rank] * S + samp(pred_off, n)[rank]
    mperm, mseg = _segments(mkey, C * S)
    gkey = gt[:, 10].long() * S + samp(gt_off, g)
    gord, gseg = _segments(gkey, C * S)
    npos = torch.bincount(gt[:, 10].long(), minlength=C).to(torch.int32)
    gcoff = (torch.cumsum(npos, 0, dtype=torch.int32) - npos).contiguous()
    max_gt = int((gseg[1:] - gseg[:-1]).max()) if g else 0
    rank, mperm, gord = rank.to(torch.int32).contiguous(), mperm.to(torch.int32).contiguous(), gord.to(torch.int32).contiguous()
    tp = torch.empty((NUSC_NTH, n), dtype=torch.int8, device=dev)
    match = torch.empty((n,), dtype=torch.int32, device=dev)
    _check(lib().u3d_nusc_match(_ptr(pred) if n else None, _ptr(rank) if n else None, _ptr(mperm) if n else None, _ptr(mseg), C * S, n,
                                _ptr(gt) if g else None, _ptr(gord) if g else None, _ptr(gseg), max_gt, _ptr(ths), tp_th,
                                _ptr(tp) if n else None, _ptr(match) if n else None, _stream()), "nusc_match")
    ws = torch.empty((int(lib().u3d_nusc_accumulate_workspace(n, g)),), dtype=torch.uint8, device=dev)
    prec = torch.empty((C, NUSC_NTH, NUSC_NI), dtype=torch.float64, device=dev)
    conf = torch.empty_like(prec)
    err = torch.empty((C, 5, NUSC_NI), dtype=torch.float64, device=dev)
    ap = torch.empty((C, NUSC_NTH), dtype=torch.float64, device=dev)
    tp_err = torch.empty((C, 5), dtype=torch.float64, device=dev)
    mri = torch.empty((C, NUSC_NTH), dtype=torch.int32, device=dev)
    nz = lambda t: _ptr(t) if t.numel() else None  # noqa: E731
    _check(lib().u3d_nusc_accumulate(nz(pred), nz(gt), nz(rank), _ptr(cseg), _ptr(npos), _ptr(gcoff), C, n, g, nz(tp), nz(match),
                                     _ptr(rec_interp), _ptr(period), tp_th, nz(ws), ws.numel(), _ptr(prec), _ptr(conf), _ptr(err), _ptr(ap),
                                     _ptr(tp_err), _ptr(mri), _stream()), "nusc_accumulate")
    return dict(rank=rank, cseg=cseg, npos=npos, tp=tp, match=match, prec=prec, conf=conf, err=err, ap=ap, tp_err=tp_err, mri=mri)


def count_tensor(n, device):
    """cached device int32 scalar holding n (row counts of static-size matrices)."""
    key = (str(device), int(n))
    t = _COUNT_CACHE.get(key)
    if t is None:
        t = torch.tensor([int(n)], dtype=torch.int32, device=device)
        _COUNT_CACHE[key] = t
    return t


def linear_bf16(x, w, bias, relu):
    """x bf16 [M,K], w bf16 [N,K] (nn.Linear layout), bias f32 [N]|None -> bf16 [M,N]; None if the shape is unsupported."""
    m, k = x.shape
    n = w.shape[0]
    if k % 64 or n % 64:
        return None
    out = torch.empty((m, n), dtype=torch.bfloat16, device=x.device)
    _check(lib().u3d_linear_bf16(_ptr(x), _ptr(w), _ptr(bias), int(relu), _ptr(out), _ptr(count_tensor(m, x.device)), m, k, n, _stream()),
           "linear_bf16")
    return out


def adamw_step(param, grad, exp_avg, exp_avg_sq, state, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=0.0, workspace=None):
    """In-place clip + AdamW on flat f32 buffers; `state` = 16 zero-initialised device floats (see include/u3d_hip.h)."""
    n = param.numel()
    wsb = int(lib().u3d_adamw_workspace(n))
    ws = workspace if workspace is not None else torch.empty(wsb, dtype=torch.uint8, device=param.device)
    _check(lib().u3d_adamw_step(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), n, lr, betas[0], betas[1], eps, weight_decay,
                                float(max_norm), _ptr(state), _ptr(ws), ws.numel(), _stream()), "adamw_step")


def adamw_set_hyper(state, lr, betas, eps, weight_decay, max_norm):
    """hyper-parameters into slots [5..10] of the 16-float device state vector (stream-ordered, one tiny launch)."""
    _check(lib().u3d_adamw_set_hyper(_ptr(state), lr, betas[0], betas[1], eps, weight_decay, float(max_norm), _stream()), "adamw_set_hyper")


def adamw_step_state(param, grad, exp_avg, exp_avg_sq, state, skip=None, workspace=None, hold=None):
    """clip + AdamW with the hyper-parameters taken from `state` (see adamw_set_hyper); skip: uint8 per 64-element chunk or None;
    hold: one device float or None - > 0 turns the step into a no-op and counts it in state[12] (capacity overflow somewhere)."""
    n = param.numel()
    wsb = int(lib().u3d_adamw_workspace(n))
    ws = workspace if workspace is not None else torch.empty(wsb, dtype=torch.uint8, device=param.device)
    _check(lib().u3d_adamw_step_hold(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), n, _ptr(state), _ptr(skip), _ptr(hold),
                                     _ptr(ws), ws.numel(), _stream()), "adamw_step_hold")


def adamw_set_accum(acc_state, accum_steps, ema_decay=None):
    """accum_steps (>= 1) and the EMA decay (None / <= 0: no EMA) into slots [0] and [4] of the 8-float device vector `acc_state`
    (stream-ordered, one tiny launch)."""
    _check(lib().u3d_adamw_set_accum(_ptr(acc_state), int(accum_steps), 0.0 if ema_decay is None else float(ema_decay), _stream()),
           "adamw_set_accum")


def adamw_step_accum(param, grad, acc, exp_avg, exp_avg_sq, state, acc_state, ema=None, skip=None, workspace=None, hold=None):
    """adamw_step_state as a MICRO-step: acc += grad, and every acc_state[0]-th call that is not held applies clip + AdamW with the
    window's mean gradient, drops the window if its norm is NaN / Inf, and moves `ema` (flat f32 or None) after an applied update.
    `acc_state` = 8 zero-initialised device floats (include/u3d_hip.h), set up with adamw_set_accum; acc_state[5] = what this call did."""
    n = param.numel()
    assert acc.numel() == n and (ema is None or ema.numel() == n) and acc_state.numel() >= 8
    wsb = int(lib().u3d_adamw_workspace(n))
    ws = workspace if workspace is not None else torch.empty(wsb, dtype=torch.uint8, device=param.device)
    _check(lib().u3d_adamw_step_accum(_ptr(param), _ptr(grad), _ptr(acc), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(ema), n, _ptr(state),
                                      _ptr(acc_state), _ptr(skip), _ptr(hold), _ptr(ws), ws.numel(), _stream()), "adamw_step_accum")


def capacity_flag(counts, caps, flag):
    """flag[0] <- number of levels with counts[i][0] > caps[i] (counts: list of device int32 tensors, caps: python ints)."""
    n = len(counts)
    assert n == len(caps) and n <= 8 and flag.dtype == torch.float32
    _check(lib().u3d_capacity_flag(_ptr_array(counts), (C.c_int32 * max(n, 1))(*[int(c) for c in caps]), n, _ptr(flag), _stream()),
           "capacity_flag")


def step_log_bytes(capacity, n_terms):
    """Bytes of a step log's row ring (u3d_step_log_bytes; 0 = refused)."""
    return int(lib().u3d_step_log_bytes(int(capacity), int(n_terms)))


def step_log_append(terms, total, opt_state, acc_state, rows, cursor):
    """One row into the step-log ring `rows` (int32 [capacity, U3D_STEP_LOG_FIXED + len(terms)]) at `cursor` (int64 [1]), on the current
    stream, capturable (u3d_step_log_append).  terms: list of device f32 scalars, total: a device f32 scalar, opt_state / acc_state
    (or None): the vectors of adamw_step_state / adamw_step_accum."""
    assert rows.dtype == torch.int32 and cursor.dtype == torch.int64 and rows.shape[1] == _K["U3D_STEP_LOG_FIXED"] + len(terms)
    assert total.dtype == torch.float32 and all(t.dtype == torch.float32 for t in terms)
    _check(lib().u3d_step_log_append(_ptr_array(terms) if terms else None, len(terms), _ptr(total), _ptr(opt_state), _ptr(acc_state),
                                     _ptr(rows), _ptr(cursor), rows.shape[0], _stream()), "step_log_append")


def step_log_window(rows, cursor, last, out, counts):
    """out f32 [columns, 4] = (mean, min, max, rows used) and counts int32 [4] = (rows seen, held, dropped, non-finite totals) of the
    latest `last` rows of a step log (u3d_step_log_window); stream-ordered, no host read."""
    n_terms = rows.shape[1] - _K["U3D_STEP_LOG_FIXED"]
    assert rows.dtype == torch.int32 and out.dtype == torch.float32 and counts.dtype == torch.int32
    assert out.numel() >= 4 * rows.shape[1] and counts.numel() >= 4
    _check(lib().u3d_step_log_window(_ptr(rows), _ptr(cursor), rows.shape[0], n_terms, int(last), _ptr(out), _ptr(counts), _stream()),
           "step_log_window")


def tap_gather_sum(p, nbr, n_dev, n, c, kvol, addend=None):
    """din[i] = sum_k p[nbr[k][i], k*c:(k+1)*c] (+ addend[i]) (f32 accumulate); p: [n_out, kvol*c]."""
    out = torch.empty((n, c), dtype=p.dtype, device=p.device)
    if addend is not None:
        assert addend.shape == out.shape and addend.dtype == out.dtype and addend.is_contiguous()
    _check(lib().u3d_tap_gather_sum(_ptr(p), _ptr(nbr), nbr.shape[1], _ptr(n_dev), n, c, kvol, dtype_code(p), _ptr(addend), _ptr(out), _stream()),
           "tap_gather_sum")
    return out


def _ptr_array(tensors):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


def _batch_chunks(outs, maxb):
    """(start, end) slices of at most maxb batch slots that never split a run of slots naming the same output tensor."""
    o, n = 0, len(outs)
    while o < n:
        e = min(n, o + maxb)
        while e < n and e > o + 1 and outs[e].data_ptr() == outs[e - 1].data_ptr():
            e -= 1
        if e < n and outs[e].data_ptr() == outs[e - 1].data_ptr():
            raise U3DError("a group of batch slots with one output is larger than the batch limit")
        yield o, e
        o = e


def wgrad_batched(ins, douts, dws):
    """dws[b] <- ins[b]^T @ douts[b] for same-shape bf16 [M,Cin] / [M,Cout] pairs (f32 [Cin,Cout] outputs, preallocated).
    CONSECUTIVE slots that name the same output are summed into it (a weight used by several layers)."""
    m, cin = ins[0].shape
    cout = douts[0].shape[1]
    dev = ins[0].device
    MAXB = 48
    for o, e in _batch_chunks(dws, MAXB):
        a, b, c = ins[o:e], douts[o:e], dws[o:e]
        wsb = int(lib().u3d_wgrad_batched_workspace(len(a), m, cin, cout))
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
        _check(lib().u3d_wgrad_batched_bf16(_ptr_array(a), _ptr_array(b), _ptr_array(c), len(a), _ptr(count_tensor(m, dev)), m, cin, cout,
                                            _ptr(ws), ws.numel(), _stream()), "wgrad_batched_bf16")


def colsum_batched(xs, outs):
    """outs[b] <- column sums of xs[b] (same-shape [n, C] matrices, f32 [C] outputs, preallocated).  CONSECUTIVE slots that name the
    same output are summed into it."""
    n, c = xs[0].shape
    dev = xs[0].device
    MAXB = 64
    for o, e in _batch_chunks(outs, MAXB):
        a, b = xs[o:e], outs[o:e]
        wsb = int(lib().u3d_colsum_batched_workspace(len(a), n, c))
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
        _check(lib().u3d_colsum_batched(_ptr_array(a), _ptr_array(b), len(a), n, c, dtype_code(a[0]), _ptr(ws), ws.numel(), _stream()),
               "colsum_batched")


def layernorm_fwd(x2, gamma, beta, eps, relu, out_dtype):
    """x2 [n, C] f32/bf16 -> (y [n, C] out_dtype, mean [n], rstd [n])."""
    n, c = x2.shape
    y = torch.empty((n, c), dtype=out_dtype, device=x2.device)
    mean = torch.empty((n,), dtype=torch.float32, device=x2.device)
    rstd = torch.empty((n,), dtype=torch.float32, device=x2.device)
    _check(lib().u3d_layernorm_fwd(_ptr(x2), dtype_code(x2), n, c, _ptr(gamma), _ptr(beta), eps, int(relu), _ptr(y), dtype_code(y),
                                   _ptr(mean), _ptr(rstd), _stream()), "layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy2, x2, gamma, beta, mean, rstd, relu):
    """-> (dx [n, C] in x2's dtype, partial f32 [2, nblocks, C] whose column sums are dgamma, dbeta)."""
    n, c = x2.shape
    dx = torch.empty_like(x2)
    nb = int(lib().u3d_layernorm_blocks(n))
    partial = torch.empty((2, nb, c), dtype=torch.float32, device=x2.device)
    _check(lib().u3d_layernorm_bwd(_ptr(dy2), dtype_code(dy2), _ptr(x2), dtype_code(x2), n, c, _ptr(gamma), _ptr(beta), _ptr(mean),
                                   _ptr(rstd), int(relu), _ptr(dx), _ptr(partial), _stream()), "layernorm_bwd")
    return dx, partial


def denormalize_boxes(codes):
    """codes [n, code>=8] f32 -> boxes [n, 7]."""
    codes = codes.contiguous()
    n, code = codes.shape
    out = torch.empty((n, 7), dtype=torch.float32, device=codes.device)
    _check(lib().u3d_denormalize_boxes(_ptr(codes), n, code, _ptr(out), _stream()), "denormalize_boxes")
    return out


def det_loss_fwd(cls, box, iou_logit, tgt, lab, w, iou_true, cls_avg, npos, code_w, alpha, w_cls, w_box, w_iou, eps):
    L, m, c = cls.shape
    code, tdim = box.shape[-1], tgt.shape[-1]
    out = torch.empty((L, 4), dtype=torch.float32, device=cls.device)
    wsb = int(lib().u3d_det_loss_workspace(L, m))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=cls.device)
    _check(lib().u3d_det_loss_fwd(_ptr(cls), _ptr(box), _ptr(iou_logit), _ptr(tgt), _ptr(lab), _ptr(w), _ptr(iou_true), _ptr(cls_avg),
                                  _ptr(npos), _ptr(code_w), L, m, c, code, tdim, alpha, w_cls, w_box, w_iou, eps, _ptr(out), _ptr(ws),
                                  ws.numel(), _stream()), "det_loss_fwd")
    return out


def det_loss_bwd(cls, box, iou_logit, tgt, lab, w, iou_true, cls_avg, npos, code_w, gout, alpha, w_cls, w_box, w_iou, eps):
    L, m, c = cls.shape
    code, tdim = box.shape[-1], tgt.shape[-1]
    dcls, dbox, diou = torch.empty_like(cls), torch.empty_like(box), torch.empty_like(iou_logit)
    _check(lib().u3d_det_loss_bwd(_ptr(cls), _ptr(box), _ptr(iou_logit), _ptr(tgt), _ptr(lab), _ptr(w), _ptr(iou_true), _ptr(cls_avg),
                                  _ptr(npos), _ptr(code_w), _ptr(gout), L, m, c, code, tdim, alpha, w_cls, w_box, w_iou, eps, _ptr(dcls),
                                  _ptr(dbox), _ptr(diou), _stream()), "det_loss_bwd")
    return dcls, dbox, diou


def skinny_wgrad_partial(dy2, x2):
    """bf16 dy2 [m, n], x2 [m, k] with min(n, k) <= 16 -> f32 [chunks, n*k] whose column sums are dW [n, k]."""
    m, n = dy2.shape
    k = x2.shape[1]
    chunks = int(lib().u3d_skinny_wgrad_chunks(m))
    partial = torch.empty((chunks, n * k), dtype=torch.float32, device=dy2.device)
    _check(lib().u3d_skinny_wgrad_bf16(_ptr(dy2), _ptr(x2), m, n, k, _ptr(partial), _stream()), "skinny_wgrad_bf16")
    return partial


def skinny_wgrad_partial_batched(dys, xs):
    """The same for a list of (dy2 [m, n_i], x2 [m, k_i]) pairs over the same m rows: one launch per skinny side (<= 32 products each).
    -> list of f32 [chunks, n_i*k_i] partials, in input order."""
    m = dys[0].shape[0]
    chunks = int(lib().u3d_skinny_wgrad_chunks(m))
    outs = [torch.empty((chunks, d.shape[1] * x.shape[1]), dtype=torch.float32, device=d.device) for d, x in zip(dys, xs)]
    for dy_skinny in (1, 0):
        sel = [i for i, (d, x) in enumerate(zip(dys, xs)) if (d.shape[1] <= x.shape[1]) == bool(dy_skinny)]
        for o in range(0, len(sel), 32):
            ii = sel[o:o + 32]
            n = (C.c_int32 * len(ii))(*[dys[i].shape[1] for i in ii])
            k = (C.c_int32 * len(ii))(*[xs[i].shape[1] for i in ii])
            _check(lib().u3d_skinny_wgrad_batched(_ptr_array([dys[i] for i in ii]), _ptr_array([xs[i] for i in ii]),
                                                  _ptr_array([outs[i] for i in ii]), n, k, len(ii), m, dy_skinny, _stream()),
                   "skinny_wgrad_batched")
    return outs


def cast_bf16(src, dst):
    """dst[i] = bf16(src[i]) over flat buffers (u3d_cast_bf16)."""
    assert src.dtype == torch.float32 and dst.dtype == torch.bfloat16 and src.numel() == dst.numel()
    _check(lib().u3d_cast_bf16(_ptr(src), _ptr(dst), C.c_int64(src.numel()), _stream()), "cast_bf16")
    return dst


PERMUTE_DESC_DTYPE = abi.numpy_dtype(_ABI.structs["u3d_permute_desc"])


PERMUTE_TILED = True


def permute_plan(descs, device):
    """descs: list of dicts with the u3d_permute_desc fields -> plan for permute_bf16_batched: descriptors whose source is contiguous
    along k go to the LDS-tiled kernel (u3d_permute_bf16_tiled), the rest to the element-wise one."""
    import numpy as np
    arr = np.zeros(len(descs), dtype=PERMUTE_DESC_DTYPE)
    per = int(lib().u3d_permute_block_elems())
    blocks, tiles, max_k = [], [], 1
    for i, d in enumerate(descs):
        for k, v in d.items():
            arr[i][k] = v
        assert d["dst_off"] % 8 == 0
        kk = d["n"] // (d["rows"] * d["cols"])
        if (PERMUTE_TILED and d["stride_k"] == 1 and d["rows"] % 32 == 0 and d["cols"] % 32 == 0 and kk <= 32 and d["src_off"] % 2 == 0
                and kk * d["rows"] * d["cols"] == d["n"] and kk in (d["stride_r"], d["stride_c"])
                and (d["stride_r"] == kk * d["cols"] or d["stride_c"] == kk * d["rows"])):
            tiles += [(i, r, c, 0) for r in range(0, d["rows"], 32) for c in range(0, d["cols"], 32)]
            max_k = max(max_k, kk)
        else:
            blocks += [(i, o) for o in range(0, d["n"], per)]
    descs_dev = torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).to(device)
    blocks_dev = torch.tensor(blocks, dtype=torch.int32).reshape(-1, 2).to(device)
    tiles_dev = torch.tensor(tiles, dtype=torch.int32).reshape(-1, 4).to(device)
    return descs_dev, blocks_dev, len(blocks), tiles_dev, len(tiles), max_k


def permute_bf16_batched(src, dst, plan):
    descs_dev, blocks_dev, nblocks, tiles_dev, ntiles, max_k = plan
    if nblocks:
        _check(lib().u3d_permute_bf16_batched(_ptr(src), _ptr(dst), _ptr(descs_dev), _ptr(blocks_dev), nblocks, _stream()), "permute_bf16_batched")
    if ntiles:
        _check(lib().u3d_permute_bf16_tiled(_ptr(src), _ptr(dst), _ptr(descs_dev), _ptr(tiles_dev), ntiles, max_k, _stream()), "permute_bf16_tiled")
    return dst


def _pc_range6(pc_range):
    return (C.c_float * 6)(*[float(v) for v in pc_range])


def box_decode_fwd(tmp, ref, pc_range, eps=1e-5):
    """tmp [n, code] f32|bf16, ref [n, 3] f32 (sigmoid space) -> decoded codes f32 [n, code] (u3d_box_decode_fwd)."""
    n, code = tmp.shape
    out = torch.empty((n, code), dtype=torch.float32, device=tmp.device)
    _check(lib().u3d_box_decode_fwd(_ptr(tmp), dtype_code(tmp), _ptr(ref), n, code, _pc_range6(pc_range), C.c_float(eps), _ptr(out), _stream()),
           "box_decode_fwd")
    return out


def refine_decode_fwd(tmp, ref_in, ref_s, pc_range, ref_out, ref_sig, eps=1e-5):
    """tmp f32 [n,code], ref_in / ref_s f32 [n,3]; ref_out / ref_sig: preallocated f32 [n,3] views -> decoded codes f32 [n,code]."""
    n, code = tmp.shape
    out = torch.empty((n, code), dtype=torch.float32, device=tmp.device)
    _check(lib().u3d_refine_decode_fwd(_ptr(tmp), _ptr(ref_in), _ptr(ref_s), n, code, _pc_range6(pc_range), C.c_float(eps), _ptr(out),
                                       _ptr(ref_out), _ptr(ref_sig), _stream()), "refine_decode_fwd")
    return out


def box_decode_bwd(tmp, ref, dout, pc_range, eps=1e-5, want_dref=False):
    n, code = tmp.shape
    dtmp = torch.empty_like(tmp)
    dref = torch.empty((n, 3), dtype=torch.float32, device=tmp.device) if want_dref else None
    _check(lib().u3d_box_decode_bwd(_ptr(tmp), dtype_code(tmp), _ptr(ref), _ptr(dout), n, code, _pc_range6(pc_range), C.c_float(eps),
                                    _ptr(dtmp), _ptr(dref), _stream()), "box_decode_bwd")
    return dtmp, dref


def sine_embed_fwd(logits, dim_t, out_dtype):
    """logits f32 [n, nc] -> [n, nc * F] in out_dtype: sin/cos embedding of sigmoid(logits) (u3d_sine_embed_fwd)."""
    n, nc = logits.shape
    F_ = dim_t.numel()
    out = torch.empty((n, nc * F_), dtype=out_dtype, device=logits.device)
    _check(lib().u3d_sine_embed_fwd(_ptr(logits), _ptr(dim_t), n, nc, F_, dtype_code(out), _ptr(out), _stream()), "sine_embed_fwd")
    return out


def sine_embed_bwd(logits, dim_t, dout):
    n, nc = logits.shape
    dl = torch.empty((n, nc), dtype=torch.float32, device=logits.device)
    _check(lib().u3d_sine_embed_bwd(_ptr(logits), _ptr(dim_t), _ptr(dout), dtype_code(dout), n, nc, dim_t.numel(), _ptr(dl), _stream()),
           "sine_embed_bwd")
    return dl


# --------------------------------------------------------------------------------------------------
# fused decoder layer (csrc/decoder.hip, csrc/decoder_bwd.hip)
# --------------------------------------------------------------------------------------------------
_SLOT_CACHE = {}
DT_F32, DT_BF16 = F32, BF16


def dt_code(dtype):
    """torch dtype of the decoder's element type -> U3D_* code."""
    if dtype == torch.bfloat16:
        return DT_BF16
    if dtype == torch.float32:
        return DT_F32
    raise U3DError(f"fused decoder: unsupported element type {dtype}")


def decoder_layer_slots(m, ncls, code, dtype=torch.bfloat16):
    """(save_off, grad_off): dicts slot name -> byte offset, plus "_total"."""
    key = (m, ncls, code, dtype)
    r = _SLOT_CACHE.get(key)
    if r is None:
        so = (C.c_int64 * (len(DS_NAMES) + 1))()
        go = (C.c_int64 * (len(DG_NAMES) + 1))()
        _check(lib().u3d_decoder_layer_slots(m, ncls, code, dt_code(dtype), so, go), "decoder_layer_slots")
        r = ({**{n: int(so[i]) for i, n in enumerate(DS_NAMES)}, "_total": int(so[len(DS_NAMES)])},
             {**{n: int(go[i]) for i, n in enumerate(DG_NAMES)}, "_total": int(go[len(DG_NAMES)])})
        _SLOT_CACHE[key] = r
    return r


def slot_view(buf, off, rows, cols, dtype):
    """[rows, cols] view of `dtype` at byte offset `off` of the uint8 buffer `buf`."""
    nbytes = rows * cols * torch.empty((), dtype=dtype).element_size()
    return buf[off:off + nbytes].view(dtype).view(rows, cols)


def decoder_blocks(m, dtype=torch.bfloat16):
    """workgroups of the row-chain kernels = rows of every LayerNorm partial matrix"""
    return int(lib().u3d_decoder_layer_blocks(m, dt_code(dtype)))


def decoder_rows(m, dtype=torch.bfloat16):
    """rows every buffer owned by the fused layer holds: m rounded up to whole row blocks (32 rows in bf16, 16 in f32: the kernels
    never branch on the row)."""
    return decoder_blocks(m, dtype) * (32 if dtype == torch.bfloat16 else 16)


def decoder_layer_fwd(params, dims, x, xc, ref, value_rows, rng, save, row_waves=0):
    """xc / value_rows / the slots are in the element type dims.dtype names (bf16 | f32); in f32 mode xc_out IS x_out.
    row_waves: waves per workgroup of the row-chain kernels (8: bf16 only | 4 | 0 = the element type's default); same bits either way."""
    m, code, ncls = dims.m, dims.code, dims.ncls
    et = torch.bfloat16 if dims.dtype == DT_BF16 else torch.float32
    assert xc.dtype == et and value_rows.dtype == et and x.dtype == torch.float32
    mp = decoder_rows(m, et)
    dev = x.device
    x_out = torch.empty((mp, 256), dtype=torch.float32, device=dev)
    xc_out = torch.empty((mp, 256), dtype=torch.bfloat16, device=dev) if et == torch.bfloat16 else x_out
    reg = torch.empty((mp, code), dtype=torch.float32, device=dev)
    cls = torch.empty((mp, ncls), dtype=torch.float32, device=dev)
    iou = torch.empty((mp,), dtype=torch.float32, device=dev)
    _check(lib().u3d_decoder_layer_fwd(C.byref(params), C.byref(dims), _ptr(x), _ptr(xc), _ptr(ref), _ptr(value_rows), _ptr(rng),
                                          _ptr(x_out), _ptr(xc_out), _ptr(reg), _ptr(cls), _ptr(iou), _ptr(save), save.numel(),
                                          int(row_waves), _stream()), "decoder_layer_fwd")
    return x_out[:m], xc_out[:m], reg[:m], cls[:m], iou[:m]


def decoder_layer_bwd(params, dims, x, xc, ref, value_rows, rng, xc_out, save, dx_out, dreg, dcls, diou, dvalue, grad, row_waves=0):
    """dvalue: f32 [rows, 256] accumulator, or (bf16 kernels only) a bf16 one: the layer's value-volume gradient is ADDED to it, summed
    per cell in a fixed order (value_scatter: bitwise reproducible).  dvalue None: nothing is scattered and the call returns
    (dx, dref, records) - the caller scatters several layers' records at once (value_scatter_layers)."""
    m = dims.m
    dims.reserved = 0
    assert dvalue is None or dvalue.dtype == torch.float32 or dims.dtype == DT_BF16
    rec = torch.empty(int(lib().u3d_value_records_bytes(m)), dtype=torch.uint8, device=ref.device)
    mp = decoder_rows(m, torch.bfloat16 if dims.dtype == DT_BF16 else torch.float32)
    dx = torch.empty((mp, 256), dtype=torch.float32, device=ref.device)
    dref = torch.empty((mp, 3), dtype=torch.float32, device=ref.device) if dims.need_dref else None
    _check(lib().u3d_decoder_layer_bwd(C.byref(params), C.byref(dims), _ptr(x), _ptr(xc), _ptr(ref), _ptr(value_rows), _ptr(rng),
                                          _ptr(xc_out), _ptr(save), _ptr(dx_out), _ptr(dreg), _ptr(dcls), _ptr(diou), _ptr(dx),
                                          _ptr(rec), _ptr(dref), _ptr(grad), grad.numel(), int(row_waves), _stream()),
           "decoder_layer_bwd")
    if dvalue is None:
        return dx[:m], (None if dref is None else dref[:m]), rec
    value_scatter(rec, m, dvalue)
    return dx[:m], (None if dref is None else dref[:m])


def value_scatter(records, m, dvalue):
    """Adds one decoder layer's value-gradient records (u3d_decoder_layer_bwd) into dvalue [cells, 256] (f32 or bf16), per cell in a
    fixed order.  The per-cell bookkeeping is scratch of this call (stream-ordered allocation, initialised by the kernel)."""
    assert dvalue.is_contiguous() and dvalue.shape[1] == 256 and dvalue.dtype in (torch.float32, torch.bfloat16)
    n = dvalue.shape[0]
    work = torch.empty(int(lib().u3d_value_scatter_workspace(n)), dtype=torch.uint8, device=dvalue.device)
    _check(lib().u3d_value_scatter(_ptr(records), m, n, _ptr(dvalue), int(dvalue.dtype == torch.bfloat16), _ptr(work), work.numel(),
                                   _stream()), "value_scatter")


VALUE_SCATTER_MAX_LAYERS = 4


def value_scatter_layers(records, ms, dvalue, order=None):
    """The records of up to VALUE_SCATTER_MAX_LAYERS decoder_layer_bwd calls into the zero-filled bf16 dvalue [cells, 256] in three
    launches (u3d_value_scatter_layers): per cell the layers' sums are added in `order` (default: as listed) - the bits of one
    value_scatter call per layer into a zeroed f32 volume, cast to bf16 afterwards."""
    assert dvalue.is_contiguous() and dvalue.shape[1] == 256 and dvalue.dtype == torch.bfloat16
    L, n = len(records), dvalue.shape[0]
    order = list(range(L)) if order is None else list(order)
    work = torch.empty(max(int(lib().u3d_value_scatter_layers_workspace(L, n)), 16), dtype=torch.uint8, device=dvalue.device)
    _check(lib().u3d_value_scatter_layers(_ptr_array(records), (C.c_int32 * L)(*ms), (C.c_int32 * L)(*order), L, n, _ptr(dvalue),
                                          _ptr(work), work.numel(), _stream()), "value_scatter_layers")


def mha_fwd(qk, v, nq, p_attn=0.0, layer=0, rng=None):
    """qk [m,512] (q | k), v [m,256] (both bf16 or both f32) -> (o [m,256] same type, lse f32 [m,8] in log2 units)."""
    m = qk.shape[0]
    assert qk.dtype == v.dtype and qk.is_contiguous() and v.is_contiguous()
    o = torch.empty((m, 256), dtype=qk.dtype, device=qk.device)
    lse = torch.empty((m, 8), dtype=torch.float32, device=qk.device)
    _check(lib().u3d_mha_fwd(_ptr(qk), _ptr(v), m, nq, p_attn, layer, _ptr(rng), _ptr(o), _ptr(lse), dt_code(qk.dtype), _stream()),
           "mha_fwd")
    return o, lse


def mha_bwd(qk, v, o, d_o, lse, nq, p_attn=0.0, layer=0, rng=None):
    m = qk.shape[0]
    assert qk.dtype == v.dtype == o.dtype == d_o.dtype
    dqk, dv = torch.empty_like(qk), torch.empty_like(v)
    _check(lib().u3d_mha_bwd(_ptr(qk), _ptr(v), _ptr(o), _ptr(d_o), _ptr(lse), m, nq, p_attn, layer, _ptr(rng), _ptr(dqk), _ptr(dv),
                                dt_code(qk.dtype), _stream()), "mha_bwd")
    return dqk, dv


def wpack(descs_dev, count, max_elems, dtype=torch.bfloat16):
    _check(lib().u3d_wpack(_ptr(descs_dev), count, max_elems, dt_code(dtype), _stream()), "wpack")


def dropout_mask(rng, layer, site, n, p, cols=0):
    """keep mask (bytes) of n elements of dropout site `site`; the attention site (4) takes cols = queries per group."""
    keep = torch.empty((n,), dtype=torch.uint8, device=rng.device)
    _check(lib().u3d_dropout_mask(_ptr(rng), layer, site, n, p, int(cols), _ptr(keep), _stream()), "dropout_mask")
    return keep


# --------------------------------------------------------------------------------------------------
# on-device data path
# --------------------------------------------------------------------------------------------------
AUG_NPARAM = _K["U3D_AUG_NPARAM"]


def points_augment(points, scene_off, params, coord, height_dim=-1):
    """In place on points [N,F] f32: per-scene flip -> rotation -> scale -> translation; params f32 [B,9]
    (flip_h, flip_v, sin, cos, angle, scale, tx, ty, tz)."""
    assert points.dtype == torch.float32 and points.is_contiguous() and params.dtype == torch.float32 and params.shape[1] == AUG_NPARAM
    batch = scene_off.numel() - 1
    _check(lib().u3d_points_augment(_ptr(points), _ptr(scene_off), batch, points.shape[0], points.shape[1], _ptr(params.contiguous()),
                                    int(coord), int(height_dim), _stream()), "points_augment")
    return points


def boxes_augment(boxes, gt_off, params, coord):
    assert boxes.dtype == torch.float32 and boxes.is_contiguous() and boxes.shape[1] in (7, 9)
    batch = gt_off.numel() - 1
    _check(lib().u3d_boxes_augment(_ptr(boxes), _ptr(gt_off), batch, boxes.shape[0], boxes.shape[1], _ptr(params.contiguous()), int(coord),
                                   _stream()), "boxes_augment")
    return boxes


def boxes_range_filter(boxes, labels, gt_off, bev_range):
    """ObjectRangeFilter in place: (boxes, labels) of every scene compacted to the front of its segment -> count int32 [B]."""
    assert boxes.dtype == torch.float32 and boxes.is_contiguous() and boxes.shape[1] in (7, 9)
    assert labels is None or (labels.dtype == torch.int32 and labels.is_contiguous())
    batch = gt_off.numel() - 1
    count = torch.empty((batch,), dtype=torch.int32, device=boxes.device)
    rng = (C.c_float * 4)(*[float(v) for v in bev_range])
    _check(lib().u3d_boxes_range_filter(_ptr(boxes), _ptr(labels), _ptr(gt_off), batch, boxes.shape[1], rng, _ptr(count), _stream()),
           "boxes_range_filter")
    return count


def points_range_filter(points, scene_off, pc_range, out=None):
    """-> (out [N,F] with every scene's survivors compacted to the front of its segment, count int32 [B])."""
    assert points.dtype == torch.float32 and points.is_contiguous()
    batch = scene_off.numel() - 1
    out = torch.empty_like(points) if out is None else out
    count = torch.empty((batch,), dtype=torch.int32, device=points.device)
    rng = (C.c_float * 6)(*[float(v) for v in pc_range])
    _check(lib().u3d_points_range_filter(_ptr(points), _ptr(scene_off), batch, points.shape[1], rng, _ptr(out), _ptr(count), _stream()),
           "points_range_filter")
    return out, count


def point_sample(points, scene_off, count, num_points, seed, want_idx=False):
    """-> out [B*num_points, F] (+ idx int32 [B*num_points]); seed: device int64/uint64 tensor with one element."""
    assert points.dtype == torch.float32 and points.is_contiguous() and seed.numel() == 1 and seed.element_size() == 8
    batch = scene_off.numel() - 1
    out = torch.empty((batch * num_points, points.shape[1]), dtype=torch.float32, device=points.device)
    idx = torch.empty((batch * num_points,), dtype=torch.int32, device=points.device) if want_idx else None
    _check(lib().u3d_point_sample(_ptr(points), _ptr(scene_off), _ptr(count), batch, points.shape[1], int(num_points), _ptr(seed), _ptr(out),
                                  _ptr(idx), _stream()), "point_sample")
    return (out, idx) if want_idx else out


def point_shuffle(points, scene_off, count, seed):
    """PointShuffle -> out [N,F]: the first count[b] rows of every scene (count None = the whole segment) permuted by a keyed
    permutation, every other row copied; seed: device int64/uint64 tensor with one element."""
    assert points.dtype == torch.float32 and points.is_contiguous() and seed.numel() == 1 and seed.element_size() == 8
    batch = scene_off.numel() - 1
    out = torch.empty_like(points)
    _check(lib().u3d_point_shuffle(_ptr(_nz(points)), _ptr(scene_off), _ptr(count), batch, points.shape[0], points.shape[1], _ptr(seed),
                                   _ptr(_nz(out)), _stream()), "point_shuffle")
    return out


def boxes_label_filter(boxes, labels, gt_off, gt_count, num_classes):
    """ObjectNameFilter in place: the live (boxes, labels) of every scene whose label is in [0, num_classes) compacted to the front of
    its segment -> count int32 [B]."""
    assert boxes.dtype == torch.float32 and boxes.is_contiguous() and boxes.shape[1] in (7, 9)
    assert labels.dtype == torch.int32 and labels.is_contiguous()
    batch = gt_off.numel() - 1
    count = torch.empty((batch,), dtype=torch.int32, device=boxes.device)
    _check(lib().u3d_boxes_label_filter(_ptr(boxes), _ptr(labels), _ptr(gt_off), _ptr(gt_count), batch, boxes.shape[1], int(num_classes),
                                        _ptr(count), _stream()), "boxes_label_filter")
    return count


# --------------------------------------------------------------------------------------------------
# batch ingest (csrc/ingest.hip)
# --------------------------------------------------------------------------------------------------
def batch_ingest(points, scene_off, count, point_cap, cat, dst_off, flag, gt=None, gt_labels=None, gt_off=None, gt_count=None, gt_cap=0,
                 gt_out=None, labels_out=None, gt_off_out=None, overflow=None):
    """A packed pipeline batch -> the caller's static buffers (u3d_batch_ingest; two launches on the current stream, no allocation, no
    host read).  points f32 [n_src, F], scene_off int32 [B+1], count int32 [B] | None -> cat f32 [B*point_cap, F] exactly packed +
    dst_off int32 [B+1]; gt f32 [g_src, 7|9] bottom-centre, gt_labels int32, gt_off, gt_count | None -> gt_out f32 [B*gt_cap, 7|9]
    gravity-centre, labels_out int32 [B*gt_cap], gt_off_out int32 [B+1] (gt None / empty with gt_out given: gt_off_out <- zeros).
    flag: one device float, += 1 when a scene was cut to a capacity; overflow: int32 [2] | None, += (points cut, boxes cut)."""
    B = scene_off.numel() - 1
    F_ = points.shape[1]
    assert points.dtype == torch.float32 and cat.dtype == torch.float32 and points.is_contiguous() and cat.shape == (B * point_cap, F_)
    assert scene_off.dtype == torch.int32 and dst_off.dtype == torch.int32 and dst_off.numel() == B + 1
    assert count is None or (count.dtype == torch.int32 and count.numel() == B)
    assert flag.dtype == torch.float32 and flag.numel() == 1 and (overflow is None or (overflow.dtype == torch.int32 and overflow.numel() == 2))
    g_src = sd = gd = 0
    if gt_out is not None:
        gd = gt_out.shape[1]
        assert gt_out.dtype == torch.float32 and gt_out.shape[0] == B * gt_cap and labels_out.dtype == torch.int32
        assert labels_out.numel() == B * gt_cap and gt_off_out.dtype == torch.int32 and gt_off_out.numel() == B + 1
    if gt is not None and gt.shape[0] > 0:
        g_src, sd = gt.shape
        assert gt_out is not None and gt.dtype == torch.float32 and gt.is_contiguous() and gt_labels.dtype == torch.int32
        assert gt_labels.numel() == g_src and gt_off.dtype == torch.int32 and gt_off.numel() == B + 1
        assert gt_count is None or (gt_count.dtype == torch.int32 and gt_count.numel() == B)
    else:
        gt = gt_labels = gt_off = gt_count = None
    _check(lib().u3d_batch_ingest(_ptr(points) if points.numel() else None, points.shape[0], F_, _ptr(scene_off), _ptr(count), B, int(point_cap), _ptr(gt), g_src, sd,
                                  _ptr(gt_labels), _ptr(gt_off), _ptr(gt_count), int(gt_cap), gd, _ptr(cat), _ptr(dst_off), _ptr(gt_out),
                                  _ptr(labels_out), _ptr(gt_off_out), _ptr(flag), _ptr(overflow), _stream()), "batch_ingest")


# --------------------------------------------------------------------------------------------------
# LoadPointsFromMultiSweeps (csrc/sweeps.hip)
# --------------------------------------------------------------------------------------------------
SWEEPS_CHUNK = _K["U3D_SWEEPS_CHUNK"]
SWEEPS_NPARAM = _K["U3D_SWEEPS_NPARAM"]     # R row-major, t, lag
SWEEP_SEG_KEY, SWEEP_SEG_SWEEP, SWEEP_SEG_PAD = _K["U3D_SWEEP_SEG_KEY"], _K["U3D_SWEEP_SEG_SWEEP"], _K["U3D_SWEEP_SEG_PAD"]


def sweeps_merge(key_points, raw, seg_tab, seg_param, seg_chunk0, scene_chunk0, n_chunks, out_rows, use_dim, remove_close):
    """-> (out [out_rows, len(use_dim)] f32, scene_off int32 [B+1]): the merged scenes exactly packed, rows past scene_off[-1] spare
    (the tables: include/u3d_hip.h u3d_sweeps_merge; all on the device, no host sync)."""
    assert key_points.dtype == torch.float32 and key_points.is_contiguous() and raw.dtype == torch.float32 and raw.is_contiguous()
    assert seg_param.dtype == torch.float64 and seg_tab.dtype == torch.int32 and seg_chunk0.dtype == torch.int32
    dev = key_points.device
    batch, n_seg, load_dim = scene_chunk0.numel() - 1, seg_tab.shape[0], key_points.shape[1]
    assert raw.numel() == 0 or raw.shape[1] == load_dim
    use = [int(d) for d in use_dim]
    out = torch.empty((max(1, int(out_rows)), len(use)), dtype=torch.float32, device=dev)
    so = torch.empty((batch + 1,), dtype=torch.int32, device=dev)
    wsb = int(lib().u3d_sweeps_merge_workspace(int(n_chunks)))
    ws = torch.empty((max(1, wsb),), dtype=torch.uint8, device=dev)
    _check(lib().u3d_sweeps_merge(_ptr(_nz(key_points)), key_points.shape[0], _ptr(_nz(raw.reshape(-1, load_dim))), raw.shape[0] if raw.numel() else 0,
                                  load_dim, _ptr(seg_tab), _ptr(seg_param), n_seg, _ptr(seg_chunk0), _ptr(scene_chunk0), batch, int(n_chunks),
                                  (C.c_int32 * len(use))(*use), len(use), int(bool(remove_close)), _ptr(ws), wsb, _ptr(out), int(out_rows),
                                  _ptr(so), _stream()), "sweeps_merge")
    return out[:int(out_rows)], so


# --------------------------------------------------------------------------------------------------
# LoadPointsFromFile / NormalizePointsColor (csrc/points_load.hip)
# --------------------------------------------------------------------------------------------------
def points_load(raw, scene_off, load_table, use_dim, shift_height):
    """-> (points [R, len(use_dim) + shift_height] f32, floor_height f32 [B] or None): the use_dim gather of the raw file rows and,
    with shift_height, the height column after the third selected one (include/u3d_hip.h u3d_points_load; no host sync)."""
    assert raw.dtype == torch.float32 and raw.dim() == 2 and raw.is_contiguous() and scene_off.dtype == torch.int32
    dev, rows, load_dim = raw.device, int(raw.shape[0]), int(raw.shape[1])
    batch = scene_off.numel() - 1
    use = [int(d) for d in use_dim]
    sh = int(bool(shift_height))
    if sh:
        assert load_table is not None and load_table.dtype == torch.float64 and load_table.numel() == 2 * batch and load_table.is_contiguous()
    out = torch.empty((rows, len(use) + sh), dtype=torch.float32, device=dev)
    floor = torch.empty((batch,), dtype=torch.float32, device=dev) if sh else None
    wsb = int(lib().u3d_points_load_workspace(rows, sh))
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev) if wsb > 0 else None
    _check(lib().u3d_points_load(_ptr(raw) if rows else None, rows, load_dim, _ptr(scene_off), batch, _ptr(load_table) if sh else None,
                                 (C.c_int32 * len(use))(*use), len(use), sh, _ptr(ws), wsb, _ptr(out) if rows else None, _ptr(floor),
                                 _stream()), "points_load")
    return out, floor


def points_color_norm(points, col0, mean=None):
    """columns col0 .. col0 + 2 of points [R, F] f32 become (c - mean) / 255.0 in place; mean None: only the division."""
    assert points.dtype == torch.float32 and points.dim() == 2 and points.is_contiguous()
    m = [0.0, 0.0, 0.0] if mean is None else [float(v) for v in mean]
    assert len(m) == 3
    rows = int(points.shape[0])
    _check(lib().u3d_points_color_norm(_ptr(points) if rows else None, rows, int(points.shape[1]), int(col0), m[0], m[1], m[2], _stream()),
           "points_color_norm")
    return points


# --------------------------------------------------------------------------------------------------
# GT-paste / ObjectNoise (csrc/objaug.hip)
# --------------------------------------------------------------------------------------------------
OA_CAP = 1024          # boxes per scene the collision / noise kernels stage in LDS


def _tiles(max_rows):
    return (int(max_rows) + 255) // 256


def _nz(t):
    """a zero-row tensor has no device pointer to hand over: one spare element instead (never read)"""
    return t if t.numel() else torch.zeros((1,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)


def objaug_stats(scene_off, count, gt_off, gt_count, labels, ncls):
    """-> int32 [2B + B*ncls] on the device: live points | live GT rows | GT rows per (scene, class)."""
    batch = scene_off.numel() - 1
    stats = torch.empty((2 * batch + batch * ncls,), dtype=torch.int32, device=scene_off.device)
    _check(lib().u3d_objaug_stats(_ptr(scene_off), _ptr(count), _ptr(gt_off), _ptr(gt_count), _ptr(_nz(labels)), batch, int(ncls), _ptr(stats),
                                  _stream()), "objaug_stats")
    return stats


def objaug_accept(gt, gt_off, g_live, db_boxes, cand_ids, cand_off, cand_grp, max_per_scene):
    """-> acc int32 [K]: 1 where the candidate survives sample_class_v2's collision rule."""
    assert gt.dtype == torch.float32 and gt.shape[1] == db_boxes.shape[1] and 0 < max_per_scene <= OA_CAP
    batch, K = gt_off.numel() - 1, cand_ids.numel()
    words = (int(max_per_scene) + 31) // 32
    acc = torch.empty((K,), dtype=torch.int32, device=gt.device)
    hit = torch.empty((K,), dtype=torch.int32, device=gt.device)
    cc = torch.empty((K * words,), dtype=torch.int32, device=gt.device)
    _check(lib().u3d_objaug_accept(_ptr(_nz(gt)), _ptr(gt_off), _ptr(g_live), gt.shape[1], _ptr(db_boxes), _ptr(cand_ids), _ptr(cand_off),
                                   _ptr(cand_grp), batch, words, _ptr(hit), _ptr(cc), _ptr(acc), _stream()), "objaug_accept")
    return acc


def points_in_boxes(points, scene_off, n_live, max_rows, boxes, box_off, box_live=None, box_active=None, max_boxes=0, want_bits=False,
                    want_tile_free=False):
    """-> (first int32 [rows], bits int32 [rows, words] or None, tile_free int32 [B, tiles] or None)."""
    assert points.dtype == torch.float32 and points.is_contiguous() and boxes.dtype == torch.float32 and boxes.shape[1] in (7, 9)
    batch, dev = scene_off.numel() - 1, points.device
    tiles = _tiles(max_rows)
    words = max(1, (int(max_boxes) + 31) // 32)
    first = torch.full((max(1, points.shape[0]),), -1, dtype=torch.int32, device=dev)
    bits = torch.zeros((max(1, points.shape[0]), words), dtype=torch.int32, device=dev) if want_bits else None
    tile_free = torch.zeros((batch, max(1, tiles)), dtype=torch.int32, device=dev) if want_tile_free else None
    _check(lib().u3d_points_in_boxes(_ptr(_nz(points)), _ptr(scene_off), _ptr(n_live), batch, points.shape[1], tiles, _ptr(_nz(boxes)),
                                     _ptr(box_off), _ptr(box_live), _ptr(box_active), boxes.shape[1], words, _ptr(first), _ptr(bits),
                                     _ptr(tile_free), _stream()), "points_in_boxes")
    return first, bits, tile_free


GTDB_MAX_BOXES = 1024  # boxes of one scene u3d_gtdb_count / u3d_gtdb_crop take


def gtdb_crop(points, scene_off, n_live, max_rows, boxes, box_off, box_valid=None, max_boxes=None):
    """Every box row becomes one database object (csrc/gtdb.hip): -> (obj_points [P, F] f32, obj_off int32 [D+1], num_points int32 [D]),
    object d = the live points of its scene strictly inside box d, in scene order, columns 0-2 relative to the box's (x, y, z_bottom).
    box_valid (int32 per box row, optional): 0 = an empty object.  max_boxes: an upper bound of the boxes of one scene if the caller
    knows one (default: all D rows; more than 1024 is an error).  Three entry points, four launches and ONE host read (the total, to
    size the output), whatever the number of scenes and boxes."""
    assert points.dtype == torch.float32 and points.is_contiguous() and boxes.dtype == torch.float32 and boxes.is_contiguous()
    assert boxes.shape[1] in (7, 9) and scene_off.dtype == torch.int32 and box_off.dtype == torch.int32
    batch, dev, feat, D = scene_off.numel() - 1, points.device, points.shape[1], boxes.shape[0]
    assert box_off.numel() == batch + 1 and (box_valid is None or (box_valid.dtype == torch.int32 and box_valid.numel() == D))
    tiles = _tiles(max_rows)
    mb = D if max_boxes is None else int(max_boxes)
    tile_ws = torch.empty((max(1, D * tiles),), dtype=torch.int32, device=dev)
    num = torch.empty((D,), dtype=torch.int32, device=dev)
    off = torch.empty((D + 1,), dtype=torch.int32, device=dev)
    total = torch.empty((1,), dtype=torch.int64, device=dev)
    geom = (_ptr(_nz(points)), points.shape[0], _ptr(scene_off), _ptr(n_live), batch, feat, tiles, _ptr(_nz(boxes)), D, _ptr(box_off),
            _ptr(box_valid), boxes.shape[1], mb)
    region = timed_begin()
    _check(lib().u3d_gtdb_count(*geom, _ptr(tile_ws), _stream()), "gtdb_count")
    timed_end(region, "gtdb_count")
    region = timed_begin()
    _check(lib().u3d_gtdb_scan(_ptr(tile_ws), D, tiles, _ptr(_nz(num)), _ptr(off), _ptr(total), _stream()), "gtdb_scan")
    timed_end(region, "gtdb_scan")
    n_out = int(total.item())                                  # the one host read
    out = torch.empty((n_out, feat), dtype=torch.float32, device=dev) if n_out < 2 ** 31 else None   # else: u3d_gtdb_crop refuses the total
    region = timed_begin()
    _check(lib().u3d_gtdb_crop(*geom, _ptr(tile_ws), _ptr(off), n_out, _ptr(_nz(out)) if out is not None else None, _stream()), "gtdb_crop")
    timed_end(region, "gtdb_crop")
    return out, off, num


def objaug_paste(points, scene_off, n_live, max_rows, gt, labels, gt_off, g_live, db_points, db_obj_off, db_boxes, db_labels, cand_ids,
                 cand_off, acc, max_obj_points, out_rows, out_box_rows, sampled_first):
    """ObjectSample's point removal + paste -> (points [out_rows, F], scene_off, boxes [out_box_rows, D], labels, gt_off): every scene
    exactly packed, the scenes back to back from row 0 (rows past scene_off[-1] / gt_off[-1] are spare capacity)."""
    batch, dev, feat, dim = scene_off.numel() - 1, points.device, points.shape[1], gt.shape[1]
    K = cand_ids.numel()
    cand_boxes = db_boxes.index_select(0, cand_ids.long()) if K else torch.zeros((0, dim), dtype=torch.float32, device=dev)
    first, _, tile_free = points_in_boxes(points, scene_off, n_live, max_rows, cand_boxes, cand_off if K else torch.zeros_like(scene_off),
                                          None, acc if K else None, want_tile_free=True)
    tiles = tile_free.shape[1]
    out_p = torch.empty((max(1, out_rows), feat), dtype=torch.float32, device=dev)
    out_b = torch.empty((max(1, out_box_rows), dim), dtype=torch.float32, device=dev)
    out_l = torch.empty((max(1, out_box_rows),), dtype=torch.int32, device=dev)
    out_so = torch.empty_like(scene_off)
    out_go = torch.empty_like(gt_off)
    tile_base = torch.empty((batch * tiles,), dtype=torch.int32, device=dev)
    cand_base = torch.empty((max(1, K),), dtype=torch.int32, device=dev)
    cand_row = torch.empty((max(1, K),), dtype=torch.int32, device=dev)
    _check(lib().u3d_objaug_paste(_ptr(_nz(points)), _ptr(scene_off), _ptr(n_live), feat, _ptr(first), _ptr(tile_free), tiles, _ptr(_nz(gt)),
                                  _ptr(_nz(labels)), _ptr(gt_off), _ptr(g_live), dim, _ptr(db_points), _ptr(db_obj_off), _ptr(db_boxes),
                                  _ptr(db_labels), _ptr(cand_ids) if K else None, _ptr(cand_off) if K else None, _ptr(acc) if K else None, K,
                                  int(max_obj_points), batch, int(bool(sampled_first)), _ptr(tile_base), _ptr(cand_base), _ptr(cand_row),
                                  _ptr(out_p), _ptr(out_so), _ptr(out_b), _ptr(out_l), _ptr(out_go), _stream()), "objaug_paste")
    return out_p[:out_rows], out_so, out_b[:out_box_rows], out_l[:out_box_rows], out_go


def object_noise(points, scene_off, n_live, max_rows, boxes, gt_off, g_live, loc, rot):
    """ObjectNoise in place on points / boxes -> chosen try per box row (int32, -1 = none)."""
    assert boxes.dtype == torch.float32 and boxes.is_contiguous() and boxes.shape[1] in (7, 9) and points.is_contiguous()
    batch, dev = scene_off.numel() - 1, points.device
    num_try = rot.shape[1]
    first = torch.empty((max(1, points.shape[0]),), dtype=torch.int32, device=dev)
    sel = torch.empty((max(1, boxes.shape[0]) * 8,), dtype=torch.float32, device=dev)
    chosen = torch.full((max(1, boxes.shape[0]),), -1, dtype=torch.int32, device=dev)
    _check(lib().u3d_object_noise(_ptr(_nz(points)), _ptr(scene_off), _ptr(n_live), batch, points.shape[1], _tiles(max_rows), _ptr(_nz(boxes)),
                                  _ptr(gt_off), _ptr(g_live), boxes.shape[1], num_try, _ptr(_nz(loc.contiguous())), _ptr(_nz(rot.contiguous())),
                                  _ptr(first), _ptr(sel), _ptr(chosen), _stream()), "object_noise")
    return chosen[:boxes.shape[0]]


# --------------------------------------------------------------------------------------------------
# Test-time augmentation: the multi-view box merge (csrc/tta.hip)
# --------------------------------------------------------------------------------------------------
TTA_LDS_CAP = _K["U3D_TTA_LDS_CAP"]     # larger (scene, class) segments take the global-memory path


def tta_inverse_params(params):
    """[V,9] forward view table (rotation + scale, then flips) -> the u3d_boxes_augment parameters of its inverse, as the merge applies
    them: (fh, fv, -sin, cos, -angle, 1/scale, 0, 0, 0)."""
    p = params.detach().float().cpu().numpy()
    inv = np.zeros_like(p)
    inv[:, 0], inv[:, 1], inv[:, 2], inv[:, 3], inv[:, 4] = p[:, 0], p[:, 1], -p[:, 2], p[:, 3], -p[:, 4]
    inv[:, 5] = np.float32(1) / p[:, 5]                   # IEEE division, as the kernel's (torch's 1 / t is a reciprocal product)
    return torch.from_numpy(inv).to(params.device)


def tta_merge(boxes, scores, labels, det_off, params, views, coord, num_classes, nms_thr=0.1, max_num=500):
    """Merge the per-view detections of B scenes (views scene-major, view-minor: det_off [B*views+1], HOST ints or a CPU tensor; a
    device tensor costs one copy to the host) -> (boxes [B, max_num, D], scores [B, max_num], labels int32 [B, max_num], count int32 [B])
    on the device, no host sync; rows past count[b] are undefined.  params: f32 [B*views, 9] forward view table (csrc/tta.hip)."""
    dev = params.device
    off_h = [int(v) for v in (det_off.cpu().tolist() if torch.is_tensor(det_off) else det_off)]
    nviews = len(off_h) - 1
    assert nviews > 0 and nviews % views == 0 and params.shape == (nviews, AUG_NPARAM)
    batch = nviews // views
    n = off_h[-1]
    dim = boxes.shape[1] if boxes.dim() == 2 else 7
    assert dim in (7, 9) and boxes.shape[0] == n and scores.shape[0] == n and labels.shape[0] == n
    max_per_scene = max(off_h[(b + 1) * views] - off_h[b * views] for b in range(batch))
    max_num = int(max_num)
    out_b = torch.empty((batch, max_num, dim), dtype=torch.float32, device=dev)
    out_s = torch.empty((batch, max_num), dtype=torch.float32, device=dev)
    out_l = torch.empty((batch, max_num), dtype=torch.int32, device=dev)
    out_c = torch.empty((batch,), dtype=torch.int32, device=dev)
    off_d = torch.tensor(off_h, dtype=torch.int32, device=dev)
    wsb = int(lib().u3d_tta_merge_workspace(n, dim, batch, int(views), int(num_classes), max_per_scene))
    ws = torch.empty((max(1, wsb),), dtype=torch.uint8, device=dev)
    b = _nz(boxes.float().contiguous().reshape(n, dim))
    sc = _nz(scores.float().contiguous())
    lb = _nz(labels.to(torch.int32).contiguous())
    _check(lib().u3d_tta_merge(_ptr(b), _ptr(sc), _ptr(lb), n, dim, _ptr(off_d), _ptr(params.float().contiguous()), batch, int(views),
                               int(coord), int(num_classes), float(nms_thr), max_num, max_per_scene, _ptr(ws), wsb, _ptr(out_b), _ptr(out_s),
                               _ptr(out_l), _ptr(out_c), _stream()), "tta_merge")
    return out_b, out_s, out_l, out_c


def tta_merge_padded(det, params, views, coord, num_classes, nms_thr=0.1, max_num=500, out=None):
    """tta_merge behind the batched tail: det is the DetBatch of B*views scenes (scene-major, view-minor) as get_bboxes_batched leaves
    it - padded [B*views, K, D] with DEVICE counts; params f32 [B*views, 9] the forward view table -> the merged DetBatch ([B, max_num,
    D], rows past count[b] zero, off written).  Scene by scene bit-identical to tta_merge on the compacted rows.  No host read, no
    synchronisation; with `out` (what an earlier call returned for the same shapes) no allocation either, so the call can be captured:
    the workspace rides on the returned batch as `out.workspace`."""
    V, K, dim = det.boxes.shape
    dev = det.boxes.device
    views, max_num = int(views), int(max_num)
    if views < 1 or V % views:
        raise U3DError(f"tta_merge_padded: {V} scenes are not a whole number of samples of {views} views")
    if det.boxes.dtype != torch.float32 or det.scores.dtype != torch.float32 or det.labels.dtype != torch.int32 or det.count.dtype != torch.int32:
        raise U3DError("tta_merge_padded takes float32 boxes / scores and int32 labels / counts")
    if det.scores.shape != (V, K) or det.labels.shape != (V, K) or det.count.numel() != V:
        raise U3DError("tta_merge_padded: boxes [V,K,D], scores / labels [V,K] and count [V] do not fit together")
    if params.dtype != torch.float32 or tuple(params.shape) != (V, AUG_NPARAM) or params.device != dev:
        raise U3DError(f"tta_merge_padded: params must be float32 [{V}, {AUG_NPARAM}] on {dev}")
    B = V // views
    wsb = int(lib().u3d_tta_merge_padded_workspace(B, views, K, dim, int(num_classes)))
    if wsb <= 0 or max_num < 1 or max_num > DET_TAIL_MAX_K:
        raise U3DError(f"tta_merge_padded: unsupported shape (B={B}, views={views}, K={K}, box_dim={dim}, num_classes={num_classes}, "
                       f"max_num={max_num} of at most {DET_TAIL_MAX_K})")
    if out is None:
        out = DetBatch(torch.empty((B, max_num, dim), dtype=torch.float32, device=dev), torch.empty((B, max_num), dtype=torch.float32, device=dev),
                       torch.empty((B, max_num), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev),
                       torch.empty((B + 1,), dtype=torch.int32, device=dev))
        out.workspace = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    ws = getattr(out, "workspace", None)
    if tuple(out.boxes.shape) != (B, max_num, dim) or ws is None or ws.numel() < wsb or out.boxes.device != dev:
        raise U3DError("tta_merge_padded: `out` was not made by a call of the same shapes")
    # named locals: a copy that .contiguous() makes must stay alive until the launch
    bx, sc, lb, ct, pr = det.boxes.contiguous(), det.scores.contiguous(), det.labels.contiguous(), det.count.contiguous(), params.contiguous()
    _check(lib().u3d_tta_merge_padded(_ptr(bx), _ptr(sc), _ptr(lb), _ptr(ct), B, views, K, dim, _ptr(pr), int(coord), int(num_classes),
                                      float(nms_thr), max_num, _ptr(ws), ws.numel(), _ptr(out.boxes), _ptr(out.scores), _ptr(out.labels),
                                      _ptr(out.count), _ptr(out.off), _stream()), "tta_merge_padded")
    return out


# --------------------------------------------------------------------------------------------------
# The batched inference tail (csrc/det_tail.hip)
# --------------------------------------------------------------------------------------------------
(DET_TAIL_NONE, DET_TAIL_NMS, DET_TAIL_DECODE, DET_TAIL_SOFT_NMS, DET_TAIL_MERGE,
 DET_TAIL_MAX_K) = (_K["U3D_DET_TAIL_" + _n] for _n in ("NONE", "NMS", "DECODE", "SOFT_NMS", "MERGE", "MAX_K"))


class DetBatch:
    """The detections of B scenes as padded tensors on one device: boxes [B,K,D], scores [B,K], labels int32 [B,K] (rows past count[b]
    are zero), count int32 [B], off int32 [B+1] = exclusive scan of count (the det_off layout of the evaluators and of tta_merge)."""

    def __init__(self, boxes, scores, labels, count, off):
        self.boxes, self.scores, self.labels, self.count, self.off = boxes, scores, labels, count, off

    def __len__(self):
        return int(self.count.shape[0])

    def cpu(self):
        """The same batch on the host: one copy per tensor."""
        return DetBatch(self.boxes.cpu(), self.scores.cpu(), self.labels.cpu(), self.count.cpu(), self.off.cpu())

    def packed(self):
        """-> (boxes [N,D], scores [N], labels int32 [N], det_off int32 [B+1]); N is read with ONE copy of off[-1] to the host."""
        n = int(self.off[-1])
        B, K, D = self.boxes.shape
        i = torch.arange(n, dtype=torch.int32, device=self.off.device)
        scene = torch.searchsorted(self.off[1:].contiguous(), i, right=True)      # empty scenes are stepped over
        row = scene * K + (i - self.off[scene])
        return self.boxes.reshape(B * K, D)[row], self.scores.reshape(-1)[row], self.labels.reshape(-1)[row], self.off

    def to_list(self):
        """-> get_bboxes' format [[boxes [n,D], scores [n], labels long [n]], ...]; ONE copy of count to the host."""
        cnt = self.count.cpu().tolist()
        lab = self.labels.long()
        return [[self.boxes[b, :c], self.scores[b, :c], lab[b, :c]] for b, c in enumerate(cnt)]

    @staticmethod
    def from_list(dets, K, dim, device):
        """Pack per-scene (boxes, scores, labels) of at most K rows each (the per-scene post-processing modes)."""
        B = len(dets)
        boxes = torch.zeros((B, K, dim), dtype=torch.float32, device=device)
        scores = torch.zeros((B, K), dtype=torch.float32, device=device)
        labels = torch.zeros((B, K), dtype=torch.int32, device=device)
        cnt = [int(d[1].shape[0]) for d in dets]
        for b, (bx, sc, lb) in enumerate(dets):
            boxes[b, :cnt[b]], scores[b, :cnt[b]], labels[b, :cnt[b]] = bx, sc, lb
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        return DetBatch(boxes, scores, labels, torch.tensor(cnt, dtype=torch.int32, device=device), torch.from_numpy(off).to(device))


def det_tail(prob, fused, boxes, max_num, center_range, score_threshold=None, mode=DET_TAIL_NONE, nms_thr=0.0, score_thr=None,
             num_thr=None, soft_sigma=0.3, soft_prune=1e-3):
    """The decode selection + post-processing of every scene in one call, no host sync (csrc/det_tail.hip; include/u3d_hip.h states
    the per-scene semantics).  prob / fused f32 [B,Q,C], boxes f32 [B,Q,7|9] gravity centre, center_range f32 [6] device tensor,
    score_thr f32 [C] device tensor or None, mode DET_TAIL_NONE / _NMS / _DECODE / _SOFT_NMS (soft_sigma, soft_prune; the scores are the
    decayed ones) / _MERGE (nms_thr is the overlap threshold; scene-wide score order) -> DetBatch with K = min(max_num, Q*C).
    All five modes go through u3d_det_tail_pp; u3d_det_tail / u3d_det_tail_workspace, the library's earlier three-mode signature kept
    for its other binders, are not called from here."""
    B, Q, Cn = prob.shape
    dim = boxes.shape[-1]
    dev = prob.device
    for t in (prob, fused, boxes, center_range) + (() if score_thr is None else (score_thr,)):
        if t.dtype != torch.float32:
            raise U3DError(f"det_tail takes float32 tensors, got {t.dtype}")
    if fused.shape != prob.shape or boxes.shape[:2] != prob.shape[:2] or center_range.numel() != 6:
        raise U3DError("det_tail: prob / fused [B,Q,C], boxes [B,Q,D] and center_range [6] do not fit together")
    if score_thr is not None and score_thr.numel() != Cn:
        raise U3DError(f"det_tail: score_thr needs one entry per class ({Cn}), got {score_thr.numel()}")
    K = min(int(max_num), Q * Cn)
    if B <= 0 or K <= 0 or K > DET_TAIL_MAX_K or dim not in (7, 9) or Q * Cn >= 2 ** 31:
        raise U3DError(f"det_tail: unsupported shape (B={B}, Q*C={Q * Cn}, K={K} of at most {DET_TAIL_MAX_K}, box_dim={dim})")
    out = DetBatch(torch.empty((B, K, dim), dtype=torch.float32, device=dev), torch.empty((B, K), dtype=torch.float32, device=dev),
                   torch.empty((B, K), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev),
                   torch.empty((B + 1,), dtype=torch.int32, device=dev))
    if mode == DET_TAIL_SOFT_NMS and not float(soft_sigma) > 0.0:
        raise U3DError(f"det_tail: soft_sigma must be positive, got {soft_sigma}")
    wsb = int(lib().u3d_det_tail_pp_workspace(B, Q, Cn, int(max_num), dim, int(mode)))
    if wsb <= 0:
        raise U3DError(f"det_tail: unknown mode {mode}")
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    # named locals: a copy that .contiguous() makes must stay alive until the launch, or the allocator hands its block to the next one
    p, f, bx, rng = prob.contiguous(), fused.contiguous(), boxes.contiguous(), center_range.contiguous()
    thr = None if score_thr is None else score_thr.contiguous()
    _check(lib().u3d_det_tail_pp(_ptr(p), _ptr(f), _ptr(bx), B, Q, Cn, dim, int(max_num), _ptr(rng), float(score_threshold or 0.0),
                                 int(mode), float(nms_thr), _ptr(thr), int(num_thr or 0), float(soft_sigma), float(soft_prune),
                                 _ptr(out.boxes), _ptr(out.scores), _ptr(out.labels), _ptr(out.count), _ptr(out.off), _ptr(ws), wsb,
                                 _stream()), "det_tail")
    return out


def det_gate(det, flag, n_live, valid=None):
    """The validity gate of a captured inference step on a finished DetBatch, in place (u3d_det_gate; two launches, no host sync):
    flag one device float (non-zero: the forward is not to be trusted), n_live one device int32 (scenes at or past it are padding)
    -> valid int32 [1] = (flag == 0); a dead scene's rows are zeroed and its count is 0, det.off is the scan of the gated counts."""
    B, K, dim = det.boxes.shape
    dev = det.boxes.device
    assert flag.dtype == torch.float32 and flag.numel() == 1 and n_live.dtype == torch.int32 and n_live.numel() == 1
    assert det.boxes.dtype == torch.float32 and det.scores.dtype == torch.float32 and det.labels.dtype == torch.int32
    assert det.scores.shape == (B, K) and det.labels.shape == (B, K)
    assert det.count.dtype == torch.int32 and det.count.numel() == B and det.off.dtype == torch.int32 and det.off.numel() == B + 1
    if valid is None:
        valid = torch.empty((1,), dtype=torch.int32, device=dev)
    assert valid.dtype == torch.int32 and valid.numel() == 1
    _check(lib().u3d_det_gate(_ptr(flag), _ptr(n_live), _ptr(det.boxes), _ptr(det.scores), _ptr(det.labels), _ptr(det.count), _ptr(det.off),
                              B, K, dim, _ptr(valid), _stream()), "det_gate")
    return valid


# --------------------------------------------------------------------------------------------------
# The device-resident detection store (csrc/det_store.hip; uni3detr_amd/det_store.py owns the buffers)
# --------------------------------------------------------------------------------------------------
def det_store_append(det, n_live, valid, scene_ids, boxes, scores, labels, table, cursor, invalid):
    """Append a DetBatch to a store's buffers (u3d_det_store_append; two launches, no host sync, capturable).  n_live / valid: one
    device int32 each or None; scene_ids int32 [B] or None (given: the repair path).  boxes [R,D], scores [R], labels int32 [R], table
    int32 [S,2], cursor int32 [4], invalid int32 [M,2] are the store.  A call that does not fit is refused on the device (cursor[3])."""
    B, K, dim = det.boxes.shape
    assert det.boxes.dtype == torch.float32 and det.scores.dtype == torch.float32 and det.labels.dtype == torch.int32
    assert det.scores.shape == (B, K) and det.labels.shape == (B, K) and det.count.dtype == torch.int32 and det.count.numel() == B
    assert boxes.dtype == torch.float32 and scores.dtype == torch.float32 and boxes.dim() == 2 and boxes.shape[1] == dim
    R, S, M = int(boxes.shape[0]), int(table.shape[0]), int(invalid.shape[0])
    assert scores.numel() == R and labels.numel() == R and labels.dtype == torch.int32
    assert table.dtype == torch.int32 and table.shape == (S, 2) and cursor.dtype == torch.int32 and cursor.numel() == 4
    assert invalid.dtype == torch.int32 and invalid.shape == (M, 2)
    for t, n in ((n_live, 1), (valid, 1), (scene_ids, B)):
        assert t is None or (t.dtype == torch.int32 and t.numel() == n)
    _check(lib().u3d_det_store_append(_ptr(det.boxes), _ptr(det.scores), _ptr(det.labels), _ptr(det.count), B, K, dim, _ptr(n_live),
                                      _ptr(valid), _ptr(scene_ids), _ptr(boxes), _ptr(scores), _ptr(labels), _ptr(table), _ptr(cursor),
                                      _ptr(invalid) if M else None, R, S, M, _stream()), "det_store_append")


def det_store_pack(boxes, scores, labels, table, n_scenes, out_rows, num_classes=0):
    """The first n_scenes scenes of a store in the evaluators' layout (u3d_det_store_pack; two launches, no host sync) ->
    (boxes [out_rows,D], scores [out_rows], labels int32 [out_rows], det_off int32 [n_scenes+1], bad int32 [2]) on the device."""
    R, dim = boxes.shape
    dev = boxes.device
    n_scenes, out_rows = int(n_scenes), int(out_rows)
    assert boxes.dtype == torch.float32 and scores.dtype == torch.float32 and labels.dtype == torch.int32 and table.dtype == torch.int32
    assert scores.numel() == R and labels.numel() == R and table.dim() == 2 and table.shape[1] == 2 and 0 <= n_scenes <= table.shape[0]
    ob = torch.empty((max(out_rows, 1), dim), dtype=torch.float32, device=dev)
    osc = torch.empty((max(out_rows, 1),), dtype=torch.float32, device=dev)
    ol = torch.empty((max(out_rows, 1),), dtype=torch.int32, device=dev)
    off = torch.empty((n_scenes + 1,), dtype=torch.int32, device=dev)
    bad = torch.empty((2,), dtype=torch.int32, device=dev)
    _check(lib().u3d_det_store_pack(_ptr(boxes), _ptr(scores), _ptr(labels), _ptr(table), n_scenes, R, dim, int(num_classes), _ptr(ob),
                                    _ptr(osc), _ptr(ol), out_rows, _ptr(off), _ptr(bad), _stream()), "det_store_pack")
    return ob[:out_rows], osc[:out_rows], ol[:out_rows], off, bad


def det_store_merge_workspace(n_scenes):
    """bytes of scratch u3d_det_store_merge wants for n_scenes mapped scenes"""
    return int(lib().u3d_det_store_merge_workspace(int(n_scenes)))


def det_store_merge(sh_boxes, sh_scores, sh_labels, sh_off, sh_head, scene_map, boxes, scores, labels, table, cursor, invalid,
                    workspace=None):
    """The shards of several ranks into a store's buffers, in the order of scene_map (u3d_det_store_merge; two launches, no host sync).
    sh_boxes [W,Nmax,D], sh_scores [W,Nmax], sh_labels int32 [W,Nmax], sh_off int32 [W,Smax+1], sh_head int32 [W,2] = (scenes, rows),
    scene_map int32 [n,2] = (shard, local scene); boxes .. invalid are the store as det_store_append takes it.  A call that does not fit
    or names what no shard holds is refused on the device (cursor[3]).  workspace: a device buffer of det_store_merge_workspace(n) bytes
    (None: allocated here)."""
    W, Nmax, dim = sh_boxes.shape
    n, Smax = int(scene_map.shape[0]), int(sh_off.shape[1]) - 1
    assert sh_boxes.dtype == torch.float32 and sh_scores.dtype == torch.float32 and sh_labels.dtype == torch.int32
    assert sh_scores.shape == (W, Nmax) and sh_labels.shape == (W, Nmax) and sh_off.dtype == torch.int32 and sh_off.shape == (W, Smax + 1)
    assert sh_head.dtype == torch.int32 and sh_head.shape == (W, 2) and scene_map.dtype == torch.int32 and scene_map.shape == (n, 2)
    assert boxes.dtype == torch.float32 and scores.dtype == torch.float32 and boxes.dim() == 2 and boxes.shape[1] == dim
    R, S, M = int(boxes.shape[0]), int(table.shape[0]), int(invalid.shape[0])
    assert scores.numel() == R and labels.numel() == R and labels.dtype == torch.int32
    assert table.dtype == torch.int32 and table.shape == (S, 2) and cursor.dtype == torch.int32 and cursor.numel() == 4
    assert invalid.dtype == torch.int32 and invalid.shape == (M, 2)
    need = det_store_merge_workspace(n)                    # (below: an empty map has no address; with n == 0 the pointer is not read)
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=boxes.device)
    _check(lib().u3d_det_store_merge(_ptr(sh_boxes), _ptr(sh_scores), _ptr(sh_labels), _ptr(sh_off), _ptr(sh_head), W, Nmax, Smax, dim,
                                     _ptr(scene_map if n else sh_head), n, _ptr(boxes), _ptr(scores), _ptr(labels), _ptr(table),
                                     _ptr(cursor), _ptr(invalid) if M else None, R, S, M, _ptr(workspace),
                                     workspace.numel() * workspace.element_size(), _stream()), "det_store_merge")
