"""Host side of the sparse levels: geometry (BitGrid / neighbour tables) and autograd wrappers around the HIP
sparse-conv / BatchNorm1d / dense() kernels.  Every op calls libu3d_hip.so; nothing here has a torch fallback.

Replaces spconv's SparseConvTensor / indice_key machinery used by the reference encoder
(ref: models/pts_encoder/sparse_encoder_hd.py:106-138).
"""
import collections
import contextlib
import os

import torch

from . import native as nv
from .shadow import conv_weights, halo_packs

K3, S1, P1 = (3, 3, 3), (1, 1, 1), (1, 1, 1)


class Level:
    """One sparse resolution: coordinates in block-major rank order + its SubM tables (built lazily, once per step —
    the reference rebuilds them for each of its 16 block convs because SparseBasicBlock carries no indice_key)."""

    def __init__(self, grid, coords, n, n_dev):
        self.grid, self.coords, self.n, self.n_dev = grid, coords, n, n_dev
        self.dims, self.batch = grid.dims, grid.batch
        self._subm = None
        self._halo = None

    def halo(self):
        """Distinct-row lists of the 128-row tiles (native.SubmHalo) for the 64 -> 64 convs of this level: built on first use."""
        if self._halo is None:
            h = nv.SubmHalo(self.subm_tables()[0], self.n_dev, self.n) if self.n <= nv.SubmHalo.MAX_ROWS else None
            self._halo = h if (h is not None and h.ok) else False      # False: too many rows for the build's LDS bitmap
        return self._halo or None

    def subm_tables(self):
        if self._subm is None:
            fwd = self.grid.nbr_table(self.coords, self.n_dev, K3, S1, P1, 0)
            # the transposed table of a SubM layer = the forward table with the offsets reversed (native.RevNbr): not built
            bwd = nv.RevNbr(fwd) if REV_SUBM_TABLE else self.grid.nbr_table(self.coords, self.n_dev, K3, S1, P1, 1)
            self._subm = (fwd, bwd)
        return self._subm


class ResidualToken:
    """Side channel between the two autograd nodes of a residual block (ref: mmdet3d SparseBasicBlock, `out += identity`): the
    BatchNorm that adds the identity deposits the identity branch's gradient here in ITS backward, and the block's first conv - whose
    backward runs later, and whose input IS the identity - sums it into its input gradient in the kernel epilogue
    (u3d_igemm_fwd_bf16 with an addend).  Autograd would add the two gradients with a separate element-wise pass over both tensors."""

    def __init__(self):
        self.dres = None


class FanoutToken:
    """Side channel between the first convs of `n` branches that take the SAME input (SECOND3D with is_cascade=False): autograd
    would add their input gradients with n - 1 element-wise passes over the full tensor.  Instead each conv's backward adds what the
    branches before it left here (kernel epilogue, u3d_igemm_fwd_bf16 with an addend) and keeps the partial sum; only the last one hands the
    total to autograd, the others return no gradient for the input."""

    def __init__(self, n, active=None):
        self.n = self.remaining = n
        self.acc = None
        self.active = active          # ActiveInput: the branches' input gradients are rows of its level ([cap, cin]), not of the lattice

    def step(self, din):
        """din already contains self.acc.  -> what this conv returns to autograd for its input."""
        self.remaining -= 1
        if self.remaining > 0:
            self.acc = din
            return None
        self.acc, self.remaining = None, self.n
        if self.active is not None:       # the total stays in the level's row order: _ToDense.backward takes it from there
            self.active.din = din
            return None
        return din


# SECOND3D's input volume is SparseEncoderHD's dense(): zero off the last level's rows (27.7 % of the cells on SUN RGB-D), and its
# gradient is read at those rows only (_ToDense.backward).  With this switch the first convolution of each SECOND3D branch computes its
# input gradient for those rows alone - the same kernels over the level's `cap` rows, through the lattice's transposed table composed
# with the level's coordinates (native.active_nbr_table) - and the stride-1 branch its weight gradient as a sum over them
# (native.spconv_wgrad_active) where ACTIVE_WGRAD allows.  bf16, FanoutToken path only; False: every launch as before.
ACTIVE_FIRST_CONV = True
# The input gradients above are bit-identical to the lattice route's at the level's rows.  The weight gradient over the level's rows is
# the same sum in another order (the level's row order and its own row splits): equal to f32 rounding (relative L2 error against float64
# 1.0e-7 vs 8.4e-8), not bit for bit - and 25 bf16 training steps carry that last-bit difference to 1e-2 in the head outputs.  Off by
# default, so that a training run reproduces its earlier self exactly; on, it takes the stride-1 launch from 127 to 44 us.
ACTIVE_WGRAD = False
_ACTIVE = [None]          # the ActiveInput of the last _ToDense.forward that wanted a gradient, until a consumer asks for it


class ActiveInput:
    """Side channel from _ToDense to the convolutions that read its volume (in the style of the tokens above): the level, its
    feature rows, and - once plugin.dense.SECOND3D has claimed it - the per-convolution tables and the total input gradient."""

    def __init__(self, lvl, feats, vol):
        self.lvl, self.feats = lvl, feats
        self.key = (vol.data_ptr(), tuple(vol.shape), vol.dtype)
        self.tables = {}          # id(ConvGeom) -> int32 [K, ld]: that convolution's transposed table over the level's rows
        self.din = None           # bf16 [cap, C]: sum of the claimed convolutions' input gradients (FanoutToken.step)

    def claim(self, geoms):
        """One batched launch for the tables of `geoms` (same lattice, same offsets)."""
        ts = nv.active_nbr_table(self.lvl.coords, self.lvl.n_dev, self.lvl.batch, self.lvl.dims, [g.nbr_bwd for g in geoms])
        self.tables = {id(g): t for g, t in zip(geoms, ts)}


def take_active(vol):
    """-> the ActiveInput whose dense() produced exactly the tensor `vol` (same storage, shape and dtype), else None.  Empties the
    side channel either way."""
    act, _ACTIVE[0] = _ACTIVE[0], None
    if act is None or not ACTIVE_FIRST_CONV or act.key != (vol.data_ptr(), tuple(vol.shape), vol.dtype):
        return None
    return act


class ConvGeom:
    """Tables of one convolution instance: forward (output-stationary), transposed (input-stationary), sizes."""

    def __init__(self, nbr_fwd, nbr_bwd, n_in, n_in_dev, n_out, n_out_dev, kind="sparse", strided=False):
        self.strided = strided      # stride > 1: bf16 dgrad = per-offset products over the output rows + gather (u3d_tap_gather_sum)
        self.nbr_fwd, self.nbr_bwd = nbr_fwd, nbr_bwd
        self.n_in, self.n_in_dev, self.n_out, self.n_out_dev = n_in, n_in_dev, n_out, n_out_dev
        self.kind = kind            # "sparse" (encoder levels) or "dense" (SECOND3D/FPN lattice): bench.py tags timings with it
        self.level = None           # SubM convs: the Level (its halo() serves the 64 -> 64 / 128 -> 128 convs, subm_halo.hip)


def level_from_coors(coors, batch, dims):
    """coors int32 [N,4] (b,z,y,x), unique.  Returns (Level, rank) with rank[i] = internal row of input row i."""
    dev = coors.device
    g = nv.BitGrid(batch, dims, dev)
    g.mark(coors)
    n = coors.shape[0]
    coords = g.scan_coords(n)
    g.set_row_capacity(n)          # unique coors => count <= n always; guards static-shape buffers all the same
    rank = g.rank(coors)
    lvl = Level(g, coords, n, g.count_dev)
    return lvl, rank


def subm_geom(lvl):
    fwd, bwd = lvl.subm_tables()
    g = ConvGeom(fwd, bwd, lvl.n, lvl.n_dev, lvl.n, lvl.n_dev)
    g.level = lvl
    return g


def strided_level(lvl, ksize, stride, pad, capacity=None):
    """Active output set + tables of a SparseConv3d (ref: sparse_encoder_hd.py:181-192).
    capacity=None: exact row count, one host read (the reference's own flow syncs at models/detectors/uni3detr.py:153).
    capacity=int : static-shape mode for hipGraph capture — tensors are sized by the capacity, every kernel is bounded by the
    device-side count, no host read (overflow is checked by the caller after the step: Level.count_dev vs capacity)."""
    dims_out = tuple((d + 2 * p - k) // s + 1 for d, k, s, p in zip(lvl.dims, ksize, stride, pad))
    g = nv.BitGrid(lvl.batch, dims_out, lvl.coords.device)
    g.mark_strided(lvl.coords, lvl.n_dev, ksize, stride, pad)
    if capacity is None:           # the row count sizes the list: scan, read it, then the coordinates
        g.scan()
        n_out = int(g.count_dev.item())
        coords = g.coords(n_out)
    else:
        n_out = int(capacity)
        coords = g.scan_coords(n_out)
        g.set_row_capacity(n_out)
    out = Level(g, coords, n_out, g.count_dev)
    fwd = lvl.grid.nbr_table(out.coords, out.n_dev, ksize, stride, pad, 0)
    bwd = g.nbr_table(lvl.coords, lvl.n_dev, ksize, stride, pad, 1)
    return out, ConvGeom(fwd, bwd, lvl.n, lvl.n_dev, n_out, out.n_dev, strided=True)


REV_SUBM_TABLE = True
SUBM_HALO = os.environ.get("U3D_SUBM_HALO", "1") == "1"       # 64 -> 64 SubM convs out of per-tile staged distinct rows (subm_halo.hip)
HALO_WGRAD = True     # ... and their weight gradients (k_subm_halo_wgrad64)
HALO_128 = True         # ... and the 128 -> 128 SubM convs (k_subm_halo128: forward / input gradient)
STRIDED_DGRAD_SPLIT = True
NMAJOR_FWD = True
STRIDED_SPLIT_MIN_RATIO = 16
STRIDED_SPLIT_SPARSE_RATIO = 16      # same threshold for the sparse levels' strided convs


_CONV_USES = {}          # id(conv weight) -> forward uses since reset_conv_uses() (TrainStep resets it at the top of every step)


def reset_conv_uses():
    _CONV_USES.clear()
    _PLANES_BWD.clear()       # (gradient planes nobody picked up in the previous step: the 4 -> 16 input conv runs on the exact f32 kernel)


# ---- split-bf16 convolutions: f32-grade products on the bf16 matrix pipe (csrc/igemm_bf16.hip: u3d_igemm_fwd_split_bf16; csrc/split_bf16.hip: the operand planes) -------------
# `mixed` precision = the REFERENCE's recipe (SparseEncoderHD + SECOND3D in fp32: sparse_encoder_hd.py:62-64, uni3detr.py:150-151).
# The exact f32 MFMA runs at 1/16 of the bf16 rate; inside split_scope() every f32 conv whose channel counts are multiples of 64 runs
# instead as three bf16 products (hi.wh + hi.wl + lo.wh, f32 accumulation) on the LDS-DMA kernels the bf16 mode is benchmarked on:
# activations travel as f32 rows, are split into hi / lo bf16 planes in front of each conv, and the three products are three sets of
# offsets of ONE launch (tripled neighbour table and weights).  Narrow levels (16 / 32 channels) stay on the exact f32 kernels.
SPLIT_BF16 = os.environ.get("U3D_SPLIT_BF16", "1") == "1"
SPLIT_FUSED_ADD = True      # residual / fan-out gradient sums in the split input gradient's epilogue
_SPLIT = [False]


# hi / lo planes that already exist for an f32 row matrix: an earlier conv split the same rows (SECOND3D's three branches read one
# input; a residual block's input feeds its first conv once).  Keyed by the tensor OBJECT (an entry holds the tensor, so the id
# cannot be reused while it lives) and its autograd version; the scope clears the table on entry and on exit, so an entry never
# outlives the forward that made it.  (Writing the planes from the BatchNorm apply that produces the rows - one pass less per layer -
# was built and measured time-neutral, 216.0 vs 217.2 scenes/s: the extra 4 B / element of stores cost what the saved read gains.)
_PLANES = {}
_PLANES_BWD = {}          # planes of a gradient tensor produced together with it (u3d_bn_bwd_apply with planes); popped by their one consumer
BN_PLANES = True          # test-only module attribute: False = every tensor is split by its own u3d_split_rows_f32 pass (the A/B formulation)


def _planes_of(feats, n_dev):
    ent = _PLANES.get(id(feats))
    if ent is not None and ent[0] is feats and ent[2] == feats._version:
        return ent[1]
    xs = nv.split_rows(feats.contiguous(), n_dev)
    if _SPLIT[0]:
        _PLANES[id(feats)] = (feats, xs, feats._version)
    return xs


def _give_planes(t, planes):
    """The BatchNorm apply pass wrote `planes` = split_rows(t) along with t: the convolution that consumes t finds them here."""
    if planes is not None and _SPLIT[0]:
        _PLANES[id(t)] = (t, planes, t._version)


def _give_bwd_planes(t, planes):
    if planes is not None:
        _PLANES_BWD[t.data_ptr()] = (t, planes, t._version)


def _bwd_planes_of(dout, n_dev):
    """bf16 planes of a convolution's output gradient: handed over by the BatchNorm backward that produced it (same storage, same
    version: the entry keeps the tensor alive, so the address cannot have been recycled), else split here."""
    ent = _PLANES_BWD.pop(dout.data_ptr(), None)
    if (ent is not None and ent[0].numel() == dout.numel() and ent[0].dtype == dout.dtype and ent[2] == ent[0]._version
            and dout.dim() == 2 and dout.is_contiguous() and ent[0].is_contiguous()):
        # (a reshaped view of the same rows - the FPN's transposed convolutions see [n, taps * C] where their BatchNorm saw
        #  [n * taps, C] - has the same planes: both are the tensor's elements in memory order, hi plane then lo plane)
        return ent[1].view(2 * dout.shape[0], dout.shape[1])
    return nv.split_rows(dout.float() if dout.dtype != torch.float32 else dout, n_dev)


@contextlib.contextmanager
def split_scope(on=True, split3=None):
    """split3: the native.Split3Set that owns the weight planes of the convolutions run inside (a detector passes its own: the job
    table and plane buffers a captured graph reads then live as long as the model); None: the module-wide default set."""
    prev, prev3 = _SPLIT[0], nv.SPLIT3_ACTIVE
    _SPLIT[0] = bool(on) and SPLIT_BF16
    _PLANES.clear()
    _PLANES_BWD.clear()
    if _SPLIT[0]:
        nv.SPLIT3_ACTIVE = split3 if split3 is not None else nv.SPLIT3_DEFAULT
        if nv.SPLIT3_BATCH:
            nv.SPLIT3_ACTIVE.refresh()          # every weight split of the step in one launch (the sets fill up during the first step)
    try:
        yield
    finally:
        _SPLIT[0] = prev
        nv.SPLIT3_ACTIVE = prev3
        _PLANES.clear()


def _split_serves(feats, cin, cout, kvol=None):
    """"wide": channels % 64 == 0 - the LDS-DMA kernels with tripled offsets; "narrow": the 27-offset 16 / 32 / 64-channel levels - three
    accumulating launches of the direct-operand kernel (kvol=None: the caller only asks about "wide"); None: the exact f32 kernels."""
    if not (_SPLIT[0] and feats.is_cuda and feats.dtype == torch.float32):
        return None
    if cin % 64 == 0 and cout % 64 == 0:
        return "wide"
    if nv.direct_serves(cin, cout, kvol):
        return "narrow"
    return None


def _split_table(geom, which, n_rows, plane):
    """int32 [3K, ld] = (t, t, t + plane): the table side - the third product reads the lo plane, `plane` rows below the hi plane.
    which: "fwd" / "bwd" / "id" (identity: a plain row product) / "wgrad" ([2K, ld] = (t, t + plane): the two products whose second
    operand is dy's hi plane).
    Cached on the geometry (static for the dense lattice; the sparse levels' geometries live for one step)."""
    owner = geom.level if (geom.level is not None and which != "id") else geom      # SubM: one set per Level, not per conv
    cache = owner.__dict__.setdefault("_split_tables", {})
    key = (which, plane)
    if key not in cache:
        t = geom.nbr_bwd if which == "bwd" else (None if which == "id" else geom.nbr_fwd)
        if t is None:                                   # 1x1x1 (or "id": a plain product over n_rows rows): the identity table
            t = torch.arange(n_rows, dtype=torch.int32, device=geom.n_out_dev.device).view(1, -1)
        elif isinstance(t, nv.RevNbr):
            t = t.t.flip(0)
        lo = torch.where(t >= 0, t + plane, t)
        cache[key] = torch.cat([t, lo] if which == "wgrad" else [t, t, lo], 0).contiguous()
    return cache[key]


def _halo_of(geom, kvol, cin, cout):
    """(The condition under which _SparseConv.forward has always picked the halo kernels, term for term, moved here so that the
    folded inference route asks the same question: tests/test_bn_fold_sparse_cpu.py pins it against the expression it replaced.)
    The level's halo tables (native.SubmHalo) when the halo kernels (subm_halo.hip) serve a bf16 conv on n-major weights: a
    27-offset SubM conv, 64 -> 64 or 128 -> 128 channels, on a level of at least 4096 rows.  Else None."""
    if not (SUBM_HALO and REV_SUBM_TABLE and geom.level is not None and kvol == 27 and cin == cout
            and (cin == 64 or (cin == 128 and HALO_128)) and geom.n_out >= 4096):
        return None
    return geom.level.halo()


# How ONE convolution runs, decided once in its forward; the backward reads the record (ctx.route) and decides nothing again.
# split: None / "wide" / "narrow" (_split_serves); nmajor: bf16 forward on the n-major weight shadow; halo: the level's halo tables
# (_halo_of) or None; strided_split: the input gradient runs as per-offset products over the output rows + u3d_tap_gather_sum.
_ConvRoute = collections.namedtuple("_ConvRoute", "split nmajor halo kvol cin cout strided_split")


def _conv_route(feats, kio_shape, geom):
    """feats: only its dtype / is_cuda are read (and the split scope and the module flags, as they stand at this call)."""
    kvol, cin, cout = kio_shape[0] * kio_shape[1] * kio_shape[2], kio_shape[3], kio_shape[4]
    bf16 = feats.dtype == torch.bfloat16
    # n-major forward weights: the LDS-DMA kernels (channels % 64) and the direct-operand kernel of the narrow 27-offset levels
    # (igemm_direct.hip stages [K][Cout][Cin] rows as they are; the k-major layout costs it a transposing prologue)
    nmajor = NMAJOR_FWD and bf16 and ((cin % 64 == 0 and cout % 64 == 0) or nv.direct_serves(cin, cout, kvol))
    split = _split_serves(feats, cin, cout, kvol)
    if split == "narrow" and geom.nbr_fwd is None:
        split = None
    halo = _halo_of(geom, kvol, cin, cout) if (nmajor and not split) else None
    # stride 4: 15/16 of the output-stationary input gradient's MFMAs hit zero rows
    strided_split = bool(STRIDED_DGRAD_SPLIT and geom.strided and kvol > 1 and (bf16 or split == "wide") and cout % 64 == 0
                         and (kvol * cin) % 64 == 0
                         and geom.n_out * (STRIDED_SPLIT_SPARSE_RATIO if geom.kind == "sparse" else STRIDED_SPLIT_MIN_RATIO) <= geom.n_in)
    return _ConvRoute(split, nmajor, halo, kvol, cin, cout, strided_split)


def _pending_addend(ctx):
    """What the tokens hold for this conv's input gradient, as the ONE tensor a kernel epilogue can take: ResidualToken.dres,
    FanoutToken.acc, their sum (formed first), or None.  The tokens keep their parts until _finish_din."""
    tok, fan = ctx.res_token, ctx.fan_token
    dres = tok.dres if tok is not None else None
    facc = fan.acc if fan is not None else None          # partial sum of the branches that ran before this one
    if dres is not None and facc is not None:
        return dres + facc
    return facc if dres is None else dres


def _finish_din(ctx, din, taken):
    """-> what the conv returns to autograd for its input.  taken: the launch that produced din already added _pending_addend(ctx);
    else the parts are added here (fan.acc, then tok.dres).  din None (no input gradient wanted): the residual token is cleared all the
    same."""
    tok, fan = ctx.res_token, ctx.fan_token
    if din is not None and not taken:
        if fan is not None and fan.acc is not None:
            din += fan.acc
        if tok is not None and tok.dres is not None:
            din = din + tok.dres
    if tok is not None:
        tok.dres = None
    return fan.step(din) if (fan is not None and din is not None) else din


class _SparseConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, weight, geom, layout, want_stats=False, res_token=None, fan_token=None):
        # weight: the PARAMETER in its checkpoint layout: "dhwio" [kD,kH,kW,Cin,Cout] (mmcv spconv-1.x) or "oidhw" (nn.Conv3d)
        # want_stats: also return the per-row-tile BatchNorm statistics of the output (empty tensor when the kernel serving this
        # shape does not produce them) - second, non-differentiable output
        ctx.set_materialize_grads(False)        # else autograd zero-fills a gradient for the statistics output on every backward
        kio_shape = weight.shape if layout == "dhwio" else tuple(weight.shape[i] for i in (2, 3, 4, 1, 0))
        if feats.shape[1] != kio_shape[3]:      # the kernels take the channel counts from the weight: a mismatch would read out of bounds
            raise ValueError(f"sparse conv: input has {feats.shape[1]} channels, weight expects {kio_shape[3]}")
        r = ctx.route = _conv_route(feats, kio_shape, geom)
        ctx.geom, ctx.layout = geom, layout
        ctx.res_token = res_token
        ctx.fan_token = fan_token if (fan_token is not None and feats.requires_grad) else None
        # the input is the dense() of a sparse level (FanoutToken.active): the backward runs over that level's rows with this table
        act = ctx.fan_token.active if ctx.fan_token is not None else None
        if act is not None and (id(geom) not in act.tables or r.split or r.halo is not None or feats.dtype != torch.bfloat16 or r.kvol == 1):
            raise RuntimeError("a fan-out token over a sparse level's rows needs every branch on the bf16 table route")   # (the sum would mix row orders)
        ctx.active = act
        # TrainStep: this parameter's slice of the flat gradient buffer - written in place by the backward ONLY if this is the
        # weight's single use in the step (a weight used twice gets two gradients that autograd must add: it may not alias them)
        _CONV_USES[id(weight)] = _CONV_USES.get(id(weight), 0) + 1
        ctx.weight_id = id(weight)
        ctx.grad_view = getattr(weight, "_u3d_grad_view", None)
        ctx.kio_shape, ctx.wdtype = kio_shape, weight.dtype
        nv.CALL_KIND = geom.kind
        out_args = (geom.n_out_dev, geom.n_out, r.cout)
        if r.split:
            xs = _planes_of(feats, geom.n_in_dev)                                        # bf16 [2 * n_in, cin]: hi | lo planes
            saved = (xs, weight)                                                         # the weight gradient reads the planes
            ctx.split3 = nv.SPLIT3_ACTIVE                                                # the backward runs outside the scope: same set
            w3 = nv.split3_weights(weight, layout, nmajor=True)                          # [3K, cout, cin], straight from the parameter
            if r.split == "narrow":
                res = nv.spconv_fwd_split_direct(xs, w3, geom.nbr_fwd, *out_args)
            else:
                res = nv.spconv_fwd_split(xs, w3, _split_table(geom, "fwd", geom.n_out, feats.shape[0]), *out_args, want_stats=want_stats)
        else:
            kio, koi = conv_weights(weight, layout, feats.dtype, want_koi=r.nmajor)
            saved = (feats, kio)
            nbr = geom.nbr_fwd if r.kvol > 1 else None
            if r.halo is not None:
                pk_fwd, ctx.pk_bwd = halo_packs(weight, kio, koi)
                res = nv.subm_halo_conv(feats, pk_fwd, r.halo, want_stats=want_stats)
            else:       # n-major: the LDS-DMA / direct-operand kernels on the n-major weight shadow (the only ones with a statistics epilogue)
                res = nv.spconv_fwd(feats, koi if r.nmajor else kio, nbr, *out_args, transpose_w=r.nmajor, tag="spconv_fwd",
                                    want_stats=want_stats and r.nmajor)
        # a launch asked for statistics: (y, stats or None, rows per tile); every other launch: y
        y, stats, tr = res if isinstance(res, tuple) else (res, None, 0)
        ctx.save_for_backward(*saved)
        if not want_stats:
            return y
        if stats is None:
            stats = torch.empty(0, dtype=torch.float64, device=feats.device)
        else:
            stats._u3d_tile_rows = tr
        ctx.mark_non_differentiable(stats)
        return y, stats

    @staticmethod
    def backward(ctx, dout, _dstats=None):
        feats, wc = ctx.saved_tensors           # (a split route: the input's bf16 planes and the parameter)
        if dout is None:
            return None, None, None, None, None, None, None
        r, g = ctx.route, ctx.geom
        dout = dout.contiguous()
        nv.CALL_KIND = g.kind
        want_din, want_dw = ctx.needs_input_grad[:2]
        din, dw, taken = None, None, False
        if r.split:
            dys = _bwd_planes_of(dout, g.n_out_dev)                                      # bf16 [2 * n_out, cout]: dy is split into planes once
            if want_dw:
                dw = _split_weight_grad(ctx, r, feats, dys)
            if want_din:
                din, taken = _split_input_grad(ctx, r, wc, dys)
        else:
            if want_dw:
                dw = _weight_grad(ctx, r, feats, dout)
            if want_din:
                din, taken = _input_grad(ctx, r, wc, dout)
        return _finish_din(ctx, din, taken), dw, None, None, None, None, None


def _weight_grad(ctx, r, feats, dout):
    g, kvol = ctx.geom, r.kvol
    nbr = g.nbr_fwd if kvol > 1 else None
    v2 = feats.dtype == torch.bfloat16 and nv.USE_IGEMM_V2 and r.cin % 16 == 0 and r.cout % 16 == 0 and ctx.wdtype == torch.float32
    # the reduction stage can write the parameter's own layout straight into its slice of the flat gradient buffer (out=):
    # autograd keeps that view as .grad and the step's packing copy has nothing to move for this parameter
    gv = ctx.grad_view if (v2 and ctx.grad_view is not None and ctx.grad_view.is_contiguous()
                           and ctx.grad_view.dtype == torch.float32 and _CONV_USES.get(ctx.weight_id, 0) == 1) else None
    if ACTIVE_WGRAD and ctx.active is not None and not g.strided and ctx.layout == "oidhw" and v2:
        # stride 1 over the dense() of a sparse level: an inactive input row is exactly zero and adds exactly zero - sum over the level's
        # rows instead, dy gathered through the transposed table.  (Strided branches: counted over active input rows, their
        # (row, offset) pairs are not fewer than over their output rows.)
        act, ks = ctx.active, ctx.kio_shape
        dw = nv.spconv_wgrad_active(dout, act.feats, act.tables[id(g)], act.lvl.n_dev, kvol, out=gv)
        return dw.view(ks[4], ks[3], ks[0], ks[1], ks[2])
    if ctx.layout == "oidhw" and v2:
        # nn.Conv3d's own [Cout,Cin,kD,kH,kW] layout: autograd keeps the tensor as the gradient
        ks = ctx.kio_shape
        return nv.spconv_wgrad(feats, dout, nbr, g.n_out_dev, kvol, out_oik=True, out=gv).view(ks[4], ks[3], ks[0], ks[1], ks[2])
    if ctx.layout == "dhwio" and v2 and r.halo is not None and HALO_WGRAD and r.cin == 64:
        return nv.subm_halo_wgrad(feats, dout, r.halo, out=gv).view(ctx.kio_shape)
    if ctx.layout == "dhwio" and v2:
        return nv.spconv_wgrad(feats, dout, nbr, g.n_out_dev, kvol, out=gv).view(ctx.kio_shape)
    dw = nv.spconv_wgrad(feats, dout, nbr, g.n_out_dev, kvol).reshape(ctx.kio_shape).to(ctx.wdtype)
    return dw.permute(4, 3, 0, 1, 2) if ctx.layout == "oidhw" else dw


def _input_grad(ctx, r, wc, dout):
    """bf16 / exact f32 input gradient -> (din, whether the launch took _pending_addend(ctx))."""
    g, kvol, cin, cout = ctx.geom, r.kvol, r.cin, r.cout
    nbr = g.nbr_bwd if kvol > 1 else None
    add = _pending_addend(ctx)
    # rows of the result: the lattice's - or, the input being the dense() of a sparse level (ctx.active), that level's `cap` rows,
    # through the transposed table composed with the level's coordinates: the same launches over 27.7 % of the rows
    n_in, n_in_dev = g.n_in, g.n_in_dev
    if ctx.active is not None:
        nbr, n_in, n_in_dev = ctx.active.tables[id(g)], ctx.active.lvl.n, ctx.active.lvl.n_dev
    fits = add is not None and add.dtype == dout.dtype and add.is_contiguous() and tuple(add.shape) == (n_in, cin)
    if r.strided_split:
        prod = nv.linear_bf16(dout, wc.view(kvol * cin, cout), None, False)      # [n_out, K*Cin]
        fan = ctx.fan_token
        if not (fits and fan is not None and add is fan.acc):                    # only the other branches' sum rides the gather
            add = None
        return nv.tap_gather_sum(prod, nbr, n_in_dev, n_in, cin, kvol, addend=add), add is not None
    if r.halo is not None:
        if not fits:
            add = None
        pk = ctx.pk_bwd if ctx.pk_bwd is not None else nv.subm_halo_wpack(wc)
        return nv.subm_halo_conv(dout, pk, r.halo, krev=True, addend=add, tag="spconv_dgrad"), add is not None
    # (an addend its epilogue cannot take - another shape or dtype, the first-generation kernel - nv.spconv_fwd adds after the launch)
    return nv.spconv_fwd(dout, wc, nbr, n_in_dev, n_in, cin, transpose_w=True, addend=add), True


def _split_weight_grad(ctx, r, xs, dys):
    """dW = x^T dy ~ xh^T dyh + xl^T dyh + xh^T dyl of a split-bf16 conv, summed in f32."""
    g, kvol = ctx.geom, r.kvol
    n_in, n_out = xs.shape[0] // 2, dys.shape[0] // 2
    if r.split == "narrow":
        # three launches of the narrow weight-gradient kernels on plane views (the table indexes rows of a plane): no doubled table
        xh, xl, dyh, dyl = xs[:n_in], xs[n_in:], dys[:n_out], dys[n_out:]
        parts = [nv.spconv_wgrad(x, dy, g.nbr_fwd, g.n_out_dev, kvol) for x, dy in ((xh, dyh), (xl, dyh), (xh, dyl))]
    else:
        # two launches of the bf16 weight-gradient kernel (offsets doubled for the two products against dy's hi plane)
        ta = _split_table(g, "wgrad", n_out, n_in)                                         # [2K, ld]: (nbr, nbr + n_in)
        a = nv.spconv_wgrad(xs, dys[:n_out], ta, g.n_out_dev, 2 * kvol)                    # [2K, cin, cout]: xh^T dyh | xl^T dyh
        b = nv.spconv_wgrad(xs, dys[n_out:], ta[:kvol], g.n_out_dev, kvol)                 # [K, cin, cout]: xh^T dyl
        parts = [a[:kvol], a[kvol:], b]
    dwk = nv.sum3(*parts).reshape(ctx.kio_shape).to(ctx.wdtype)
    return dwk.permute(4, 3, 0, 1, 2) if ctx.layout == "oidhw" else dwk


def _split_input_grad(ctx, r, wc, dys):
    """dx of a split-bf16 conv: three products as in the forward (transposed tables / weights) -> (din, whether the launch took
    _pending_addend(ctx))."""
    g, kvol, cin, cout = ctx.geom, r.kvol, r.cin, r.cout
    n_out = dys.shape[0] // 2
    w3 = nv.split3_weights(wc, ctx.layout, nmajor=False, cache=ctx.split3)
    if r.split == "narrow":
        return nv.spconv_fwd_split_direct(dys, w3, g.nbr_bwd, g.n_in_dev, g.n_in, cin, tag="spconv_dgrad"), False
    if r.strided_split:
        # strided conv: per-offset products over the (few) OUTPUT rows - one split product with the identity table, [n_out, K * Cin]
        # f32 - then the gather over the offsets that reach each input row (as the bf16 path, u3d_tap_gather_sum; the
        # output-stationary form runs all K x 3 products for every input row, 15/16 of them on absent neighbours at stride 4)
        tid = _split_table(g, "id", n_out, n_out)
        wt3 = w3.view(3, kvol * cin, cout)                                                 # [K, Cin, Cout] as ONE [K * Cin, Cout] matrix
        prod = nv.spconv_fwd_split(dys, wt3, tid, g.n_out_dev, n_out, kvol * cin, tag="spconv_dgrad")
        return nv.tap_gather_sum(prod, g.nbr_bwd, g.n_in_dev, g.n_in, cin, kvol), False
    # the residual branch's / the other fan-out branches' gradient rides the launch's epilogue (f32 addend), as in bf16 mode
    add = _pending_addend(ctx) if SPLIT_FUSED_ADD else None
    if add is not None and not (add.dtype == torch.float32 and add.is_contiguous() and tuple(add.shape) == (g.n_in, cin)):
        add = None
    t3 = _split_table(g, "bwd", g.n_in, n_out)
    return nv.spconv_fwd_split(dys, w3, t3, g.n_in_dev, g.n_in, cin, tag="spconv_dgrad", addend=add), add is not None


def sparse_conv(feats, weight, geom, layout="dhwio", fan_token=None):
    """weight: conv PARAMETER in checkpoint layout ("dhwio" = [kD,kH,kW,Cin,Cout]; "oidhw" = nn.Conv3d's [Cout,Cin,kD,kH,kW])."""
    return _SparseConv.apply(feats, weight, geom, layout, False, None, fan_token)


FUSED_CONV_STATS = True


# ---- inference: eval-mode BatchNorm folded into the convolution (uni3detr_amd/inference.py) ---------------------------------------------
# Inside fold_scope(table) a conv_bn() call whose BatchNorm module is in `table` (id(bn) -> FoldedPair, the records an InferenceModel
# owns) runs on the kernel the record's `route` names, conv_folded(); every other call, and every call outside a scope, is what it
# always was.
_FOLD = [None]


@contextlib.contextmanager
def fold_scope(table):
    prev = _FOLD[0]
    _FOLD[0] = table
    try:
        yield
    finally:
        _FOLD[0] = prev


class FoldedPair:
    """One folded conv + BatchNorm pair of an InferenceModel.  name / weight / layout / bn: the convolution's module path, its f32
    parameter in its checkpoint layout and the BatchNorm module - what refresh() folds from; sparse_level: a pair only
    InferenceModel(sparse_levels=True) folds.  allocate() adds the buffers and fixes the route: w_folded bf16 [kvol, Cout, Cin], shift
    f32 [Cout] (native.BnFoldTable) and w_packed, w_folded in the halo kernels' fragment order or None.  A pair of
    InferenceModel(dense_fp8=True) also has qw uint8 [kvol, Cout, Cin] e4m3 codes and e_w int32 [Cout] (native.BnFoldFp8Table, which
    writes the same `shift`), e_a: the activation exponent as a device int32 [1] (what the quantise pass reads) and colscale f32 [Cout]
    = 2^(e_a + e_w), both set by calibration, which runs on w_folded, and slot: this layer's f32 absmax slot.
    route     the kernel, and what becomes of a residual (a block's conv2)
    "affine"  LDS-DMA affine (nv.igemm_fwd_affine); a residual is an error
    "direct"  direct-operand affine (nv.igemm_direct_affine), which takes the residual
    "halo"    nv.subm_halo_conv_affine, which takes the residual, where the level's halo tables serve the call (_halo_of: the one
              decision left to the call); else as "level"
    "level"   LDS-DMA affine: every other sparse-level pair (ScanNet-large's 256-channel block convs).  With a residual conv_folded()
              -> None and conv_bn runs conv + u3d_bn_apply: the LDS-DMA kernels take a shift OR an addend
    "fp8"     conv_affine_fp8, or while calibrating absmax_rows + the LDS-DMA affine launch on w_folded; a residual is an error"""
    __slots__ = ("name", "weight", "layout", "bn", "sparse_level", "route", "w_folded", "shift", "w_packed",
                 "qw", "e_w", "e_a", "colscale", "slot", "calibrating", "calibrated")

    def __init__(self, name, weight, layout, bn, sparse_level):
        self.name, self.weight, self.layout, self.bn, self.sparse_level = name, weight, layout, bn, sparse_level
        self.route = self.w_folded = self.shift = self.w_packed = None
        self.qw = self.e_w = self.e_a = self.colscale = self.slot = None
        self.calibrating = self.calibrated = False

    def allocate(self, halo_conv, fp8=None):
        """The buffers, on the parameter's device, and the route.  halo_conv: a SubM conv (the halo kernels serve 27 offsets, 64 -> 64 /
        128 -> 128 of them); fp8: None or (e_a, slot), this layer's views of the model-wide tables."""
        dev = self.weight.device
        k, cout, cin = nv.conv_weight_strides(tuple(self.weight.shape), self.layout)[:3]
        self.w_folded = torch.empty((k, cout, cin), dtype=torch.bfloat16, device=dev)
        self.shift = torch.empty((cout,), dtype=torch.float32, device=dev)
        packed = self.sparse_level and halo_conv and k == 27 and cin == cout and cin in (64, 128)
        self.w_packed = torch.empty_like(self.w_folded) if packed else None
        self.route = ("fp8" if fp8 else "affine" if not self.sparse_level else "halo" if packed
                      else "direct" if nv.direct_serves(cin, cout, k) else "level")
        if fp8:
            self.qw = torch.empty((k, cout, cin), dtype=torch.uint8, device=dev)
            self.e_w = torch.zeros((cout,), dtype=torch.int32, device=dev)
            self.colscale = torch.zeros((cout,), dtype=torch.float32, device=dev)
            self.e_a, self.slot = fp8


def _inference_input(what, feats, w, geom, residual=None):
    """The input checks of the inference path, for its three launch paths.  w: the pair's weights or codes, [kvol, Cout, Cin]."""
    if torch.is_grad_enabled() and (feats.requires_grad or w.requires_grad or (residual is not None and residual.requires_grad)):
        raise RuntimeError(f"{what} is an inference path: it records no autograd node")
    if feats.dtype != torch.bfloat16 or not feats.is_cuda:
        raise RuntimeError(f"{what} needs bf16 device rows, got {feats.dtype} on {feats.device}")
    if feats.shape[1] != w.shape[2]:
        raise ValueError(f"{what}: input has {feats.shape[1]} channels, folded weight expects {w.shape[2]}")
    if residual is not None and not (residual.dtype == torch.bfloat16 and tuple(residual.shape) == (geom.n_out, w.shape[1])):
        raise ValueError(f"{what}: the residual must be bf16 rows of the output's shape")


def conv_affine(feats, w_folded, shift, geom, relu=True):
    """relu(conv(feats; w_folded) + shift) in one launch (u3d_igemm_fwd_affine_bf16): conv -> eval-mode BatchNorm -> ReLU with the
    BatchNorm's scale folded into the bf16 n-major weights [kvol, Cout, Cin] and its shift kept in f32 (native.bn_fold).  Inference
    only (no autograd node); bf16 rows, channels % 64 == 0 - anything else is an error, not a detour."""
    _inference_input("conv_affine", feats, w_folded, geom)
    nv.CALL_KIND = geom.kind
    nbr = geom.nbr_fwd if w_folded.shape[0] > 1 else None
    return nv.igemm_fwd_affine(feats.contiguous(), w_folded, nbr, shift, relu, geom.n_out_dev, geom.n_out)


def conv_affine_fp8(feats, ent, geom, relu=True):
    """relu(conv(q(feats); qw) * colscale + shift) in two launches: the bf16 input rows are quantised to e4m3 under the layer's
    calibrated exponent (u3d_quant_rows_e4m3), then the fp8 convolution runs (u3d_igemm_fwd_affine_fp8).  Inference only; bf16 rows,
    a shape native.fwd_fp8_plan serves - anything else is an error, not a detour."""
    _inference_input("conv_affine_fp8", feats, ent.qw, geom)
    if not ent.calibrated:
        raise RuntimeError(f"fp8 layer {ent.name} has no activation scale yet: run InferenceModel.calibrate() or load_fp8_state() first")
    nv.CALL_KIND = geom.kind
    qin = nv.quant_rows_e4m3(feats.contiguous(), ent.e_a, geom.n_in_dev)
    nbr = geom.nbr_fwd if ent.qw.shape[0] > 1 else None
    return nv.igemm_fwd_affine_fp8(qin, ent.qw, nbr, ent.colscale, ent.shift, relu, geom.n_out_dev, geom.n_out)


def conv_folded(feats, ent, geom, residual=None, relu=True):
    """relu(conv(feats; w_folded) + shift + residual) of a FoldedPair on its route's kernel (the table in its docstring).  -> None
    where no kernel has the epilogue: the caller then runs conv + u3d_bn_apply."""
    if ent.route == "fp8" and not ent.calibrating:
        return conv_affine_fp8(feats, ent, geom, relu)
    _inference_input("a folded conv + BatchNorm pair", feats, ent.w_folded, geom, residual)
    kvol, cout, cin = ent.w_folded.shape
    halo = _halo_of(geom, kvol, cin, cout) if ent.route == "halo" else None
    if residual is not None and halo is None and ent.route != "direct":
        return None
    feats, add = feats.contiguous(), None if residual is None else residual.contiguous()
    nv.CALL_KIND = geom.kind
    if halo is not None:
        return nv.subm_halo_conv_affine(feats, ent.w_packed, halo, ent.shift, relu, add)
    if ent.route == "direct":
        return nv.igemm_direct_affine(feats, ent.w_folded, geom.nbr_fwd, ent.shift, relu, geom.n_out_dev, geom.n_out, add)
    if ent.route == "fp8":
        nv.absmax_rows(feats, geom.n_in_dev, ent.slot)      # calibration: the bf16 folded forward + this layer's input range
    return nv.igemm_fwd_affine(feats, ent.w_folded, geom.nbr_fwd if kvol > 1 else None, ent.shift, relu, geom.n_out_dev, geom.n_out)


def conv_bn(feats, weight, geom, bn, n_dev, residual=None, relu=True, layout="dhwio", post_add=None, res_take=None, res_give=None, fan_token=None):
    """conv -> BatchNorm rows (+ residual) (+ ReLU).  In training the conv's epilogue already reduces the BatchNorm statistics per row
    tile where its kernel supports it (bf16, channels % 64 == 0): the separate statistics pass over the conv output disappears."""
    if _FOLD[0] is not None:
        ent = _FOLD[0].get(id(bn))
        if ent is not None:
            if bn.training or post_add is not None or (residual is not None and not ent.sparse_level):
                what = "an fp8 conv + BatchNorm pair" if ent.route == "fp8" else "a folded conv + BatchNorm pair"
                raise RuntimeError(f"{what} of a sparse level was called in training mode, or with a level sum" if ent.sparse_level else
                                   f"{what} was called in training mode, or with a residual / level sum")
            y = conv_folded(feats, ent, geom, residual, relu)
            if y is not None:
                return y
    if _conv_stats_serve(feats, bn):
        # res_take: this conv's input is the identity of a residual block - its backward sums the token's gradient into the input
        # gradient; res_give: this BatchNorm adds that identity - its backward leaves the identity's gradient in the token
        # fan_token: this conv is one of several that take the same input (FanoutToken)
        y, stats, tr = conv_with_stats(feats, weight, geom, layout, res_take, fan_token)
        if stats is not None:
            return _BNRows.apply(y, bn.weight, bn.bias, residual, n_dev, bn, relu, True, stats, tr, None, post_add, res_give)
        return _BNRows.apply(y, bn.weight, bn.bias, residual, n_dev, bn, relu, bn.training, None, 0, None, post_add, res_give)
    return bn_rows(sparse_conv(feats, weight, geom, layout, fan_token), bn, n_dev, residual, relu, None, post_add)


def _conv_stats_serve(feats, bn):
    """The convolution in front of a training-mode BatchNorm is asked for the statistics of its output."""
    return bool(FUSED_CONV_STATS and bn.training and feats.is_cuda
                and (feats.dtype == torch.bfloat16 or _split_serves(feats, feats.shape[1], bn.num_features) == "wide"))


def conv_with_stats(feats, weight, geom, layout, res_take=None, fan_token=None):
    """-> (y, stats, rows per tile): the conv with the BatchNorm statistics of y reduced per row tile in its epilogue (what
    native.bn_finalize_partials takes), or (y, None, 0) where the kernel serving the shape does not produce them."""
    y, stats = _SparseConv.apply(feats, weight, geom, layout, True, res_take, fan_token)
    if not stats.numel():
        return y, None, 0
    tr = getattr(stats, "_u3d_tile_rows", None)
    if tr is None:                      # attribute lost on the way through autograd: recover it from the shape
        nb = stats.shape[0]
        tr = next((t for t in (128, 256, 192) if (y.shape[0] + t - 1) // t == nb), 0)
    return y, stats, tr


class _BNRows(torch.autograd.Function):
    """BatchNorm1d over active rows (+ residual) (+ ReLU), training or eval statistics."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, n_dev, bn, relu, training, stats=None, tile_rows=0, row_map=None, post_add=None, res_token=None):
        n = x.shape[0]
        if training and stats is not None:
            mean, invstd = nv.bn_finalize_partials(stats, tile_rows, n_dev, n, bn.eps, bn.momentum if bn.momentum is not None else 0.1,
                                                   bn.running_mean, bn.running_var, bn.num_batches_tracked)
        elif training:
            mean, invstd = nv.bn_forward_stats(x, n_dev, bn.eps, bn.momentum if bn.momentum is not None else 0.1,
                                               bn.running_mean, bn.running_var, bn.num_batches_tracked)
        else:
            mean = bn.running_mean
            invstd = torch.rsqrt(bn.running_var + bn.eps)
        g32, b32 = gamma.float(), beta.float()
        if post_add is not None:
            assert relu and residual is None and post_add.shape == x.shape and post_add.dtype == x.dtype
            post_add = post_add.contiguous()
        # split-bf16 scope, f32 rows: the pass also writes y's hi / lo bf16 planes for the convolution that reads y next, and the backward
        # will write the planes of dx for the convolution that produced x (the planes argument of u3d_bn_apply / u3d_bn_bwd_apply)
        ctx.planes = bool(BN_PLANES and _SPLIT[0] and x.is_cuda and x.dtype == torch.float32 and x.shape[1] % 16 == 0)
        if ctx.planes:
            y, ypl = nv.bn_apply(x, mean, invstd, g32, b32, residual, relu, n_dev, row_map, post_add, want_planes=True)
            _give_planes(y, ypl)
        else:
            y = nv.bn_apply(x, mean, invstd, g32, b32, residual, relu, n_dev, row_map, post_add)
        # ReLU without residual: the backward recomputes the mask from x (same expression) instead of streaming y again
        ctx.remask = bool(relu and residual is None)
        ctx.save_for_backward(x, None if ctx.remask else y, mean, invstd, g32, b32)
        ctx.n_dev, ctx.relu, ctx.training, ctx.has_res = n_dev, relu, training, residual is not None
        ctx.pdtype = gamma.dtype
        ctx.row_map = row_map
        ctx.has_post = post_add is not None
        ctx.res_token = res_token if residual is not None else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, mean, invstd, gamma, beta = ctx.saved_tensors
        dy = dy.contiguous()
        sums, s32 = nv.bn_bwd_stats(dy, y, x, mean, invstd, ctx.relu, ctx.n_dev, gamma, beta, ctx.row_map, want_f32=True)
        use = sums if ctx.training else torch.zeros_like(sums)       # eval statistics are constants: dx = gamma*invstd*g
        if ctx.planes:
            dx, dres, dpl = nv.bn_bwd_apply(dy, y, x, mean, invstd, gamma, use, ctx.relu, ctx.n_dev, ctx.has_res, beta, ctx.row_map, want_planes=True)
            _give_bwd_planes(dx, dpl)
        else:
            dx, dres = nv.bn_bwd_apply(dy, y, x, mean, invstd, gamma, use, ctx.relu, ctx.n_dev, ctx.has_res, beta, ctx.row_map)
        if ctx.pdtype != torch.float32:
            s32 = s32.to(ctx.pdtype)
        if ctx.res_token is not None and dres is not None:
            ctx.res_token.dres, dres = dres, None            # picked up by the block's first conv (ResidualToken)
        # post_add enters y by a plain sum: its gradient is dy itself (no launch)
        return dx, s32[1], s32[0], dres, None, None, None, None, None, None, None, (dy if ctx.has_post else None), None


def bn_rows(x, bn, n_dev, residual=None, relu=True, row_map=None, post_add=None):
    """row_map: the output (and its gradient) use a permuted row order, y[row_map[r]] = bn(x[r]) - see u3d_bn_apply."""
    return _BNRows.apply(x, bn.weight, bn.bias, residual, n_dev, bn, relu, bn.training, None, 0, row_map, post_add, None)


def bn_rows_sum_serves(levels, c, params):
    """native.bn_apply_sum / bn_bwd_apply_sum take this level count, width and these column parameters (u3d_bn_apply_sum's
    preconditions, asked before the statistics run: a refusal afterwards could not be undone)."""
    return (2 <= levels <= 4 and c % 8 == 0 and 256 % (c // 8) == 0 and levels * 6 * c * 4 <= 64 * 1024
            and all(p.dtype != torch.float32 or p.data_ptr() % 16 == 0 for p in params))


class _BNRowsSum(torch.autograd.Function):
    """sum_i relu(BatchNorm_i(x_i)) over levels that land on one lattice, training statistics, bf16 rows: the chain of _BNRows nodes
    with post_add (plugin.dense.SECOND3DFPN) as ONE node.  Statistics as in _BNRows, level by level (the conv's partials or a pass over
    x_i; the backward's three passes with row_map); one apply launch forward and one backward instead of one per level - the partial
    sums are neither written nor read again, and dout is read once.  Bit-identical to the chain.
    specs[i] = (bn, stats or None, tile_rows, idx or None, inv or None): idx maps a lattice row to the row of x_i, inv is its inverse
    (Lattice.upsample_index); tensors = x_0, gamma_0, beta_0, x_1, ..."""

    @staticmethod
    def forward(ctx, n_dev, specs, *tensors):
        xs, gammas, betas = tensors[0::3], tensors[1::3], tensors[2::3]
        n = xs[0].shape[0]
        means, invstds = [], []
        for x, (bn, stats, tile_rows, _, _) in zip(xs, specs):
            mom = bn.momentum if bn.momentum is not None else 0.1
            if stats is not None:
                mean, invstd = nv.bn_finalize_partials(stats, tile_rows, n_dev, n, bn.eps, mom, bn.running_mean, bn.running_var,
                                                       bn.num_batches_tracked)
            else:
                mean, invstd = nv.bn_forward_stats(x, n_dev, bn.eps, mom, bn.running_mean, bn.running_var, bn.num_batches_tracked)
            means.append(mean)
            invstds.append(invstd)
        g32, b32 = [g.float() for g in gammas], [b.float() for b in betas]
        idxs = [s[3] for s in specs]
        out = nv.bn_apply_sum(xs, means, invstds, g32, b32, idxs, n_dev)
        if out is None:
            raise nv.U3DError("bn_apply_sum refused a shape bn_rows_sum_serves() let through")
        ctx.save_for_backward(*xs, *means, *invstds, *g32, *b32)
        ctx.n_dev, ctx.idxs, ctx.invs = n_dev, idxs, [s[4] for s in specs]
        ctx.pdtypes = [g.dtype for g in gammas]
        return out

    @staticmethod
    def backward(ctx, dout):
        L = len(ctx.idxs)
        t = ctx.saved_tensors
        xs, means, invstds, gammas, betas = (t[i * L:(i + 1) * L] for i in range(5))
        dout = dout.contiguous()
        # the sum's gradient w.r.t. every level is dout itself; the mask of each level's ReLU is recomputed from x_i (_BNRows' remask)
        stats = [nv.bn_bwd_stats(dout, None, xs[i], means[i], invstds[i], True, ctx.n_dev, gammas[i], betas[i], ctx.invs[i], want_f32=True)
                 for i in range(L)]
        dxs = nv.bn_bwd_apply_sum(dout, xs, means, invstds, gammas, betas, [s[0] for s in stats], ctx.idxs, ctx.n_dev)
        grads = []
        for i in range(L):
            s32 = stats[i][1] if ctx.pdtypes[i] == torch.float32 else stats[i][1].to(ctx.pdtypes[i])
            grads += [dxs[i], s32[1], s32[0]]
        return (None, None, *grads)


def bn_rows_sum(xs, bns, n_dev, stats, idxs, invs):
    """stats[i]: (partials, rows per tile) of the conv that produced xs[i] (conv_with_stats), or None."""
    specs = [(bn, None if st is None else st[0], 0 if st is None else st[1], idx, inv) for bn, st, idx, inv in zip(bns, stats, idxs, invs)]
    flat = [t for x, bn in zip(xs, bns) for t in (x, bn.weight, bn.bias)]
    return _BNRowsSum.apply(n_dev, specs, *flat)


class _ToDense(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, lvl):
        ctx.lvl = lvl
        vol = nv.to_dense(feats, lvl.coords, lvl.n_dev, lvl.batch, lvl.dims)
        ctx.active = _ACTIVE[0] = None
        if ACTIVE_FIRST_CONV and ctx.needs_input_grad[0] and feats.dtype == torch.bfloat16 and feats.is_cuda:
            ctx.set_materialize_grads(False)    # the readers may hand their gradient over in row order (ActiveInput.din): dvol = None
            ctx.active = _ACTIVE[0] = ActiveInput(lvl, feats, vol)
        return vol

    @staticmethod
    def backward(ctx, dvol):
        lvl, act = ctx.lvl, ctx.active
        din = None
        if act is not None:
            din, act.din, act.feats = act.din, None, None
        if dvol is not None:                               # (whatever read the volume besides the claimed convolutions - or all of it)
            cl = dvol.permute(0, 2, 3, 4, 1).contiguous()      # no copy when dvol is channels_last_3d
            rows = nv.from_dense(cl, lvl.coords, lvl.n_dev, lvl.n)
            din = rows if din is None else din + rows
        return din, None


def to_dense(feats, lvl):
    """rows -> [B,C,D,H,W] (channels_last_3d memory) (ref: sparse_encoder_hd.py:133)."""
    vol = _ToDense.apply(feats, lvl)
    act = _ACTIVE[0]
    if act is not None and act.key == (vol.data_ptr(), tuple(vol.shape), vol.dtype):
        vol._u3d_active = act          # for dense_backward(): a backward cut at this volume
    return vol


def dense_backward(vol, gvol):
    """vol.backward(gvol) for a backward that was cut at a to_dense() volume (TrainStep's phased backward: the readers saw a detached
    leaf, gvol = its gradient).  gvol is None when the readers left their input gradient in the level's row order instead
    (ActiveInput.din): the encoder's backward then starts from the level's rows - the dense() node has nothing left to do."""
    act = getattr(vol, "_u3d_active", None)
    if gvol is None and act is not None and act.din is not None:
        feats, din, act.feats, act.din = act.feats, act.din, None, None
        feats.backward(din)
        return
    vol.backward(gvol)


class _PermuteRows(torch.autograd.Function):
    """out[rank[i]] = in[i] (API row order -> internal block-major order)."""

    @staticmethod
    def forward(ctx, feats, rank, n_out):
        ctx.save_for_backward(rank)
        return nv.scatter_rows(feats.contiguous(), rank, n_out)

    @staticmethod
    def backward(ctx, dout):
        (rank,) = ctx.saved_tensors
        return nv.gather_rows(dout.contiguous(), rank), None, None


def permute_rows(feats, rank, n_out):
    return _PermuteRows.apply(feats, rank, n_out)
