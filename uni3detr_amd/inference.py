"""Inference with eval-mode BatchNorm folded into the convolutions (bf16 mode).

In eval mode a BatchNorm is a constant per-channel affine map, y = x * scale + shift.  `model.eval()` still runs it as its own pass
(`u3d_bn_apply`): conv -> BatchNorm -> ReLU is two launches and three trips over the activation tensor, plus a cast and a re-layout
of the f32 master weight per conv and forward.  InferenceModel multiplies the scale into a bf16 copy of the weights once (ONE launch
for the whole model, native.bn_fold) and hands the shift to the epilogue of the implicit-GEMM kernels (sparse.conv_affine): one
launch, one trip, no per-forward weight cast.

    model.set_precision("bf16").eval()
    inf = InferenceModel(model)                          # or InferenceModel(model, sparse_levels=True), see below
    det = inf.simple_test_batched(img_metas, points, on_device=True)
    inf.refresh()            # after parameters or running statistics changed
    inf.folded, inf.unfolded

What folds by default: every conv + BatchNorm (+ ReLU) pair whose channel counts are multiples of 64 and whose BatchNorm does nothing
else - all of SECOND3D, the FPN's extra_blocks and its first level when that is a plain convolution, and in SparseEncoderHD the strided
64 / 128-channel convolutions and conv_out.  What keeps conv + u3d_bn_apply by default, exactly as under model.eval() (`inf.unfolded`
names each layer and the reason):
  * conv_input (a padded 4 / 5-channel input on its own kernel);
  * the narrow sparse levels (16 / 32 channels) and the SubM residual blocks of the 64- / 128-channel levels: the plain entries of
    the direct-operand and halo kernels take an addend but no shift, and a block's second BatchNorm also adds the identity - these
    are what sparse_levels=True folds, below;
  * the FPN's transposed-conv levels and every level after the first: their BatchNorm apply carries the lattice permutation
    (row_map) and the running level sum (post_add) for free.
sparse_levels=True (off by default) also folds the rest of SparseEncoderHD: every SparseBasicBlock conv and the narrow strided
convs.  The halo kernels and the direct-operand kernels have an affine instantiation for it (shift, then the block's identity as the
addend, then ReLU, one rounding: u3d_subm_halo_conv64 / 128_affine_bf16, u3d_igemm_direct_affine_bf16), and refresh() packs the folded
64- / 128-channel weights into the halo kernels' fragment order once (one batched launch per channel count) instead of once per conv
and forward.  conv_input and the FPN entries above stay unfolded.  A folded pair is one record (sparse.FoldedPair) whose `route` - halo
kernel, direct-operand kernel, the LDS-DMA affine kernel - is fixed by shape when its buffers are allocated; a call decides only
whether the level's halo tables serve it (sparse._halo_of).  ONE case falls back to conv + u3d_bn_apply exactly as model.eval() runs
it: the conv2 of a 64- / 128- / 256-channel block on a level the halo kernels do not serve (fewer than 4096 rows, more rows than
the halo build's bitmap holds, or 256 channels as in ScanNet-large's last stage).  Its BatchNorm adds the identity, and the LDS-DMA
kernels take a shift or an addend, not both.  Such a layer is listed in `folded` (its weights are folded; conv1 of the same block takes
the LDS-DMA affine kernel) and costs its u3d_bn_apply launch on the levels where it falls back.

The model itself is not changed: the folded route is taken only inside InferenceModel's own scope (sparse.fold_scope), and
`model.simple_test*` called directly stays the unfolded yardstick.

dense_fp8=True (off by default) runs the wide dense convolutions of SECOND3D and the FPN on OCP e4m3 operands (sparse.conv_affine_fp8:
a quantise pass over the bf16 input rows, then u3d_igemm_fwd_affine_fp8 on the block-scaled MFMA).  Weights are folded and quantised per
output channel from the f32 masters, activations per layer under a power-of-two scale that calibrate(batches) measures on a bf16 folded
forward (fp8_state() / load_fp8_state() carry it).  `fp8_layers` names the pairs on that route - those the fp8 launch plan serves and that
measured faster than bf16 -, `fp8_skipped` the rest with the reason.  A forward before calibration raises.  INTEGRATION.md N.

InferenceStep(inf, batch_size=B, point_capacity=P) replays the folded forward and the batched tail of an InferenceModel as one hipGraph
over static, capacity-sized buffers, with a device-side validity gate (u3d_det_gate) and an eager fallback.  INTEGRATION.md O.  With
views=A it captures test-time augmentation as well: B * A views forward, the multi-view merge on the padded tail.  INTEGRATION.md S.
It serves dynamic voxelization (ScanNet-large, DynamicSimpleVFE) too: a capacity-sized voxel list and, inside scope(), order-free voxel
means, so that a replay and its eager fallback compute the same bits.  INTEGRATION.md T.

Numerics: not bit-identical to conv + u3d_bn_apply.  Folded: bf16(w * scale) once, output rounded once.  Unfolded: bf16(w), conv
output rounded to bf16, y rounded.  Both are a few bf16 roundings of the same real number (tests/test_bn_fold_gpu.py holds the folded
error within 2 x the unfolded one against a float64 restatement).
"""
import contextlib
import math

import torch
from torch import nn

from . import native as nv
from . import sparse as sp
from . import static_batch as sb
from .tta import coord_of as _coord_of

_WHY_NARROW = "narrow level ({cin} -> {cout} channels): direct-operand kernels read `bias` as an addend"
_WHY_INPUT = "conv_input: {cin} -> {cout} channels on its own kernel"
_WHY_BLOCK = "SubM residual block: the halo kernels have no shift epilogue (conv2's BatchNorm also adds the identity)"
_WHY_DECONV = "transposed conv: its BatchNorm apply carries the lattice permutation (row_map) and the level sum (post_add)"
_WHY_LEVEL = "FPN level sum rides this BatchNorm apply (post_add)"


def _wide(cin, cout):
    return cin % 64 == 0 and cout % 64 == 0


def classify(model, sparse_levels=False):
    """-> (folded, unfolded): folded = [(name, weight parameter, layout, BatchNorm module)], unfolded = [(name, reason)], in forward
    order.  `name` is the convolution's module path.  Needs no device.  sparse_levels: also fold SparseEncoderHD's block convs and
    narrow strided convs (input channels % 4 == 0: what the fold kernel writes)."""
    folded, unfolded = _classify(model, sparse_levels)
    return [p[:4] for p in folded], unfolded


def _classify(model, sparse_levels):
    """classify(), each folded pair with a fifth item: whether it is one that only sparse_levels folds (FoldedPair.sparse_level)."""
    from .plugin.dense import SECOND3D, SECOND3DFPN
    from .plugin.sparse_encoder import SparseBasicBlock, SparseEncoderHD
    names = {id(m): n for n, m in model.named_modules()}
    folded, unfolded = [], []

    def pair(conv, bn, weight, layout, cin, cout, why=None, sparse_level=False):
        name = names[id(conv)]
        if why is None and not _wide(cin, cout):
            why = _WHY_NARROW.format(cin=cin, cout=cout)
        # what only sparse_levels folds: on the halo / direct-operand affine kernels, else the LDS-DMA one (sparse.conv_folded)
        only_sparse = bool(why is not None and sparse_level and sparse_levels and cin % 4 == 0)
        if only_sparse:
            why = None
        if why is None and not (isinstance(bn, nn.modules.batchnorm._BatchNorm) and bn.affine and bn.track_running_stats):
            why = "BatchNorm without affine parameters or running statistics"
        if why is None:
            folded.append((name, weight, layout, bn, only_sparse))
        else:
            unfolded.append((name, why))

    enc = getattr(model, "pts_middle_encoder", None)
    if isinstance(enc, SparseEncoderHD):
        c = enc.conv_input[0]
        pair(c, enc.conv_input[1], c.weight, "dhwio", c.cin, c.cout, _WHY_INPUT.format(cin=c.cin, cout=c.cout))
        for stage in enc.encoder_layers:
            for m in stage:
                if isinstance(m, SparseBasicBlock):
                    for conv, bn in ((m.conv1, m.bn1), (m.conv2, m.bn2)):
                        pair(conv, bn, conv.weight, "dhwio", conv.cin, conv.cout, _WHY_BLOCK if _wide(conv.cin, conv.cout) else None, True)
                else:
                    pair(m[0], m[1], m[0].weight, "dhwio", m[0].cin, m[0].cout, None, True)
        c = enc.conv_out[0]
        pair(c, enc.conv_out[1], c.weight, "dhwio", c.cin, c.cout)
    elif enc is not None:
        raise TypeError(f"InferenceModel knows SparseEncoderHD, not {type(enc).__name__}")
    bb = getattr(model, "pts_backbone", None)
    if isinstance(bb, SECOND3D):
        for blk in bb.blocks:
            mods = list(blk)
            for j in range(0, len(mods), 3):
                pair(mods[j], mods[j + 1], mods[j].weight, "oidhw", mods[j].in_channels, mods[j].out_channels)
    elif bb is not None:
        raise TypeError(f"InferenceModel knows SECOND3D, not {type(bb).__name__}")
    neck = getattr(model, "pts_neck", None)
    if isinstance(neck, SECOND3DFPN):
        for i, d in enumerate(neck.deblocks):
            if isinstance(d[0], nn.ConvTranspose3d):
                unfolded.append((names[id(d[0])], _WHY_DECONV))
            else:
                pair(d[0], d[1], d[0].weight, "oidhw", d[0].in_channels, d[0].out_channels, _WHY_LEVEL if i > 0 else None)
        if neck.extra_conv is not None:
            mods = list(neck.extra_blocks)
            for j in range(0, len(mods), 3):
                pair(mods[j], mods[j + 1], mods[j].weight, "oidhw", mods[j].in_channels, mods[j].out_channels)
    elif neck is not None:
        raise TypeError(f"InferenceModel knows SECOND3DFPN, not {type(neck).__name__}")
    return folded, unfolded


_FP8_DENSE = ("pts_backbone.", "pts_neck.")
_WHY_FP8_SCOPE = "not a dense-stack layer: SparseEncoderHD stays bf16"


def fp8_exponent(x):
    """The smallest integer e with x <= 448 * 2^e, i.e. ceil(log2(x / 448)), computed exactly (x = m * 2^k, 448 = 0.875 * 2^9); 0 for
    x == 0.  The activation exponent of a layer is fp8_exponent(amax * headroom), a weight channel's fp8_exponent(max |w_folded|)."""
    if not (x >= 0.0 and math.isfinite(x)):
        raise ValueError(f"fp8_exponent: {x!r} is not a finite non-negative number")
    if x == 0.0:
        return 0
    m, k = math.frexp(x)
    return k - 9 if m <= 0.875 else k - 8


def _fp8_slower(cin, cout, kvol, stride):
    """The layer kinds the kernel serves but the quantise pass + fp8 convolution does not run faster than the bf16 launch, with the
    measured pair of times (ms, medians, MI355X, 192 000 input rows: profiles/fp8_inference_layer_ab.txt); None: fp8 is faster."""
    if stride > 1:
        return (f"strided ({cin} -> {cout}, stride {stride}): the quantise pass walks every input row, {stride * stride} x the output rows - "
                "measured quant + fp8 0.066 ms vs bf16 0.061 ms (stride 2, within the spread), 0.059 vs 0.046 ms (stride 4)")
    if kvol == 1:
        return (f"1 x 1 x 1 ({cin} -> {cout}): memory-bound, the fp8 kernel alone ties the bf16 one and the quantise pass comes on top - "
                "measured quant + fp8 0.072 ms vs bf16 0.054 ms")
    if cin == 128 and cout == 128:
        return ("128 -> 128 channels: half of the 256-column tile is masked and a k-tile is the whole input row - measured quant + fp8 "
                "0.078 ms vs bf16 0.077 ms (within the spread; at KITTI's 704 000 rows 0.282 vs 0.289 ms, 1.03 x, faster beyond the spread: skipped there too, this rule does not see the row count)")
    return None


def classify_fp8(model, pairs=None):
    """-> (fp8, skipped): fp8 = names of the default-fold pairs of SECOND3D / SECOND3DFPN that the fp8 launch plan serves
    (native.fwd_fp8_plan: Cin % 128 == 0, Cout % 128 == 0) and that measured faster than bf16 (_fp8_slower), skipped = [(name, reason)]
    for every other folded pair.  Needs the built library but no device (the plan query is host only)."""
    pairs = classify(model)[0] if pairs is None else pairs
    mods = dict(model.named_modules())
    fp8, skipped = [], []
    for name, w, layout, _ in pairs:
        kvol, cout, cin = nv.conv_weight_strides(tuple(w.shape), layout)[:3]
        if not name.startswith(_FP8_DENSE):
            skipped.append((name, _WHY_FP8_SCOPE))
        elif nv.fwd_fp8_plan(1 << 16, cin, cout, kvol, kvol > 1) is None:
            skipped.append((name, f"the fp8 launch plan does not serve {cin} -> {cout} channels, {kvol} offsets (channels % 128)"))
        else:
            why = _fp8_slower(cin, cout, kvol, max(getattr(mods[name], "stride", (1,))))
            if why is None:
                fp8.append(name)
            else:
                skipped.append((name, why))
    return fp8, skipped


def _sources(r):
    """The f32 tensors a record is folded from: the conv weight and the BatchNorm's parameters and running statistics."""
    return r.weight, r.bn.weight, r.bn.bias, r.bn.running_mean, r.bn.running_var


def _fold_job(r, *destinations):
    """A record as a row of native.BnFoldTable / BnFoldFp8Table."""
    return (r.weight.detach(), r.layout, r.bn.weight.detach(), r.bn.bias.detach(), r.bn.running_mean, r.bn.running_var, r.bn.eps) + destinations


class InferenceModel:
    """A Uni3DETR in eval mode and bf16 precision with its foldable BatchNorms folded away.  Owns the folded weights and shifts;
    the wrapped model keeps its parameters, its state_dict and its own (unfolded) eval path.

    dense_fp8=True (off by default) runs the wide dense convolutions (SECOND3D, SECOND3DFPN: `fp8_layers`; the rest with the reason in
    `fp8_skipped`) on e4m3 operands: weights folded and quantised per output channel, activations quantised per layer under a
    power-of-two scale that calibrate() measures once (or load_fp8_state() restores).  Until then a forward raises RuntimeError."""

    def __init__(self, model, sparse_levels=False, dense_fp8=False):
        if model.training:
            raise RuntimeError("InferenceModel folds eval-mode BatchNorm: call model.eval() first")
        prec = getattr(model, "precision", None)
        if prec != "bf16":
            raise ValueError(f"InferenceModel folds into bf16 weights: set_precision('bf16') first (the model is in {prec!r} mode, "
                             "which keeps the unfolded path)")
        self.model = model
        self.sparse_levels = bool(sparse_levels)
        folded, unfolded = _classify(model, self.sparse_levels)
        self._records = [sp.FoldedPair(*p) for p in folded]      # in forward order; their buffers and routes: _allocate()
        self.folded = [r.name for r in self._records]
        self.unfolded = list(unfolded)
        self._table, self._sig = None, None
        self._by_bn = {}          # id(BatchNorm module) -> record: what sparse.fold_scope takes; empty until the buffers exist
        self._fp8 = []            # the records on the fp8 route, in fp8_layers order
        self._packs = None
        self.dense_fp8 = bool(dense_fp8)
        default_pairs = [(r.name, r.weight, r.layout, r.bn) for r in self._records if not r.sparse_level]
        self.fp8_layers, self.fp8_skipped = classify_fp8(model, default_pairs) if self.dense_fp8 else ([], [])
        self.fp8_headroom = None
        self._fp8_e_a, self._fp8_table, self._fp8_sig = None, None, None
        if self._records and self._records[0].weight.is_cuda:
            self._allocate()
            self.refresh()

    @property
    def fp8_calibrated(self):
        return self.fp8_headroom is not None

    def _fp8_scales(self):
        """colscale[c] = 2^(e_a + e_w[c]) of every fp8 layer, on the device, into the buffers the entries already point at."""
        for ent in self._fp8:
            ent.colscale.copy_(torch.ldexp(torch.ones_like(ent.colscale), ent.e_w + ent.e_a))
            ent.calibrated = True

    def calibrate(self, batches, headroom=2.0):
        """Measure the activation range of every fp8 layer: the bf16 folded forward runs over `batches` (an iterable of point lists,
        what extract_pts_feat takes) and takes the running max |input| of each layer on the device (no host sync inside a forward);
        then ONE read of the slots, e_a = ceil(log2(amax * headroom / 448)) per layer (headroom 2 = one binade: free in relative
        precision, larger run-time values saturate), and the column scales.  -> {name: (amax, e_a)}.  A zero or non-finite amax
        raises with the layer's name."""
        if not self.dense_fp8:
            raise RuntimeError("InferenceModel.calibrate: the model was not wrapped with dense_fp8=True")
        if not self._by_bn:
            raise RuntimeError("InferenceModel: the model was not on the device when it was wrapped; move it there and call refresh()")
        if not (headroom >= 1.0 and math.isfinite(headroom)):
            raise ValueError(f"calibrate: headroom must be a finite number >= 1, got {headroom!r}")
        self._fp8_slots.zero_()
        for ent in self._fp8:
            ent.calibrating = True
        try:
            for points in batches:
                self._extract(points)
        finally:
            for ent in self._fp8:
                ent.calibrating = False
        amax = self._fp8_slots.tolist()
        out, e_a = {}, []
        for ent, a in zip(self._fp8, amax):
            if not (math.isfinite(a) and a > 0.0):
                raise ValueError(f"calibrate: fp8 layer {ent.name} saw max |input| = {a!r} (no calibration data reached it, or a non-finite activation)")
            e_a.append(fp8_exponent(a * headroom))
            out[ent.name] = (a, e_a[-1])
        if e_a:
            self._fp8_e_a.copy_(torch.tensor(e_a, dtype=torch.int32))
        self.fp8_headroom = float(headroom)
        self._fp8_scales()
        return out

    def fp8_state(self):
        """What calibration found, as plain Python: {"headroom": h, "e_a": {layer name: exponent}} (load_fp8_state restores it)."""
        if not self.fp8_calibrated:
            raise RuntimeError("InferenceModel.fp8_state: not calibrated")
        return {"headroom": self.fp8_headroom, "e_a": dict(zip(self.fp8_layers, self._fp8_e_a[:len(self._fp8)].tolist()))}

    def load_fp8_state(self, state):
        """Restore activation exponents saved by fp8_state(): no calibration forward.  The layer names must be this model's."""
        if not self.dense_fp8:
            raise RuntimeError("InferenceModel.load_fp8_state: the model was not wrapped with dense_fp8=True")
        if set(state["e_a"]) != set(self.fp8_layers):
            raise ValueError("load_fp8_state: the saved layers are not this model's fp8 layers")
        if not self._by_bn:
            raise RuntimeError("InferenceModel: the model was not on the device when it was wrapped; move it there and call refresh()")
        if self._fp8:
            self._fp8_e_a.copy_(torch.tensor([int(state["e_a"][n]) for n in self.fp8_layers], dtype=torch.int32))
        self.fp8_headroom = float(state["headroom"])
        self._fp8_scales()
        return self

    def _allocate(self):
        """Every record's buffers and route (sparse.FoldedPair.allocate).  An fp8 layer keeps its bf16 buffers: w_folded stays resident for
        later calibrations, and both fold launches of a refresh() write the same values into `shift` (one formula, one f32 evaluation
        order in both kernels).  The activation exponents and absmax slots of all fp8 layers are one tensor each (read once)."""
        from .plugin.sparse_encoder import SparseConvWeight
        halo_convs = {id(m.weight) for m in self.model.modules() if isinstance(m, SparseConvWeight) and m.subm} if self.sparse_levels else ()
        dev = self._records[0].weight.device
        if self.dense_fp8:
            e_a = self._fp8_e_a        # (kept across a move to another device: calibration is not repeated)
            self._fp8_e_a = torch.zeros((max(len(self.fp8_layers), 1),), dtype=torch.int32, device=dev) if e_a is None else e_a.to(dev)
            self._fp8_slots = torch.zeros((max(len(self.fp8_layers), 1),), dtype=torch.float32, device=dev)
        for r in self._records:
            i = self.fp8_layers.index(r.name) if r.name in self.fp8_layers else None
            r.allocate(id(r.weight) in halo_convs, None if i is None else (self._fp8_e_a[i:i + 1], self._fp8_slots[i:i + 1]))
        self._by_bn = {id(r.bn): r for r in self._records}
        self._fp8 = [r for r in self._records if r.route == "fp8"]
        assert [r.name for r in self._fp8] == self.fp8_layers
        self._packs = self._fp8_table = None

    def refresh(self):
        """Fold again: after an optimizer step, load_state_dict or a change of the running statistics.  One launch - with
        sparse_levels, one more per channel count (64, 128) that packs the folded block weights for the halo kernels; the job table
        and the pack plans are rebuilt only when a parameter or buffer moved in memory."""
        if not self._records:
            return self
        dev = self._records[0].weight.device
        if not self._by_bn or self._records[0].w_folded.device != dev:
            self._allocate()
            self._table = None
        sig = tuple(t.data_ptr() for r in self._records for t in _sources(r))
        if self._table is None or sig != self._sig:
            if any(t.dtype != torch.float32 for r in self._records for t in _sources(r)):
                raise TypeError("InferenceModel folds from f32 master parameters and statistics")
            self._table, self._sig = nv.BnFoldTable([_fold_job(r, r.w_folded, r.shift) for r in self._records]), sig
        self._table.run()
        if self._fp8:
            # the fp8 layers again from the f32 masters (one rounding, not the bf16 copy rounded again): ONE more launch; the channel
            # exponents may have moved, so the column scales follow
            if self._fp8_table is None or sig != self._fp8_sig:
                self._fp8_table, self._fp8_sig = nv.BnFoldFp8Table([_fold_job(r, r.qw, r.e_w, r.shift) for r in self._fp8]), sig
            self._fp8_table.run()
            if self.fp8_calibrated:
                self._fp8_scales()
        if self._packs is None:
            by_c = {}
            for r in self._records:
                if r.w_packed is not None:
                    by_c.setdefault(r.w_folded.shape[1], []).append((r.w_folded, r.w_packed))
            self._packs = [nv.subm_halo_wpack_plan(by_c[c], dev) for c in sorted(by_c)]
        for plan in self._packs:
            nv.subm_halo_wpack_batched(plan)
        return self

    @contextlib.contextmanager
    def scope(self, calibrating=False):
        """Inside: the wrapped model's forward takes the folded route, under bf16 autocast.  Refuses training mode and enabled
        gradients - and, with fp8 layers, a forward before calibration (calibrating: calibrate()'s own forward)."""
        if self.model.training:
            raise RuntimeError("InferenceModel: the model went back to training mode")
        if torch.is_grad_enabled():
            raise RuntimeError("InferenceModel: gradients are enabled - the folded forward records no autograd graph (use torch.no_grad())")
        if self.fp8_layers and not calibrating and not self.fp8_calibrated:
            raise RuntimeError("InferenceModel(dense_fp8=True): no activation scales yet - run calibrate(batches) or load_fp8_state() first")
        if not self._by_bn:
            raise RuntimeError("InferenceModel: the model was not on the device when it was wrapped; move it there and call refresh()")
        # dynamic voxelization: order-free voxel means inside the scope, so that a captured replay, its eager fallback and a second
        # replay of the same points compute the same bits (outside it the encoder keeps its f32 atomics)
        vfe = getattr(self.model, "pts_voxel_encoder", None)
        order_free = hasattr(vfe, "exact_mean")
        prev = vfe.exact_mean if order_free else None
        if order_free:
            vfe.exact_mean = True
        try:
            # the head runs under bf16 autocast, as Uni3DETR.forward_pts_train runs it in this mode (the fused decoder takes bf16 rows)
            with sp.fold_scope(self._by_bn), torch.autocast("cuda", dtype=torch.bfloat16):
                yield self
        finally:
            if order_free:
                vfe.exact_mean = prev

    @torch.no_grad()
    def _extract(self, points):
        with self.scope(calibrating=True):
            return self.model.extract_pts_feat(points)

    @torch.no_grad()
    def extract_pts_feat(self, points):
        with self.scope():
            return self.model.extract_pts_feat(points)

    @torch.no_grad()
    def head_outputs(self, points, img_metas=None):
        """The detection head's raw outputs (all_cls_scores, all_bbox_preds, ...) of the folded forward."""
        with self.scope():
            feat, fps = self.model.extract_pts_feat(points)
            return self.model.pts_bbox_head(feat, img_metas, fps)

    @torch.no_grad()
    def simple_test(self, img_metas, points=None, rescale=False):
        with self.scope():
            return self.model.simple_test(img_metas, points, rescale=rescale)

    @torch.no_grad()
    def simple_test_batched(self, img_metas, points=None, rescale=False, on_device=False):
        with self.scope():
            return self.model.simple_test_batched(img_metas, points, rescale=rescale, on_device=on_device)

    @torch.no_grad()
    def aug_test(self, points, img_metas, **kwargs):
        with self.scope():
            return self.model.aug_test(points, img_metas, **kwargs)

    @torch.no_grad()
    def aug_test_batched(self, batch_or_points, img_metas=None, **kwargs):
        """Uni3DETR.aug_test_batched on the folded route: one forward over all views, the batched tail and the padded merge on the device."""
        with self.scope():
            return self.model.aug_test_batched(batch_or_points, img_metas, **kwargs)


class InferenceStep:
    """The folded forward and the batched tail of an InferenceModel as ONE hipGraph over static buffers: a batch costs one replay
    instead of a few hundred enqueued launches.

        step = InferenceStep(inf, batch_size=B, point_capacity=P)
        counts, caps = step.capture(batches=[pts_a, pts_b, ...], margin=1.25, warmup=3)
        det = step.run(points)        # native.DetBatch in the graph's static buffers; step.valid (int32 [1]) says whether to read it
        res = step.results(points)    # simple_test_batched's list of dicts on the host; the eager path when the replay was invalid
        step.valid, step.fallbacks, step.overflows()

    Inputs are a static_batch.StaticBatch without GT: `cat` f32 [B * P, F] of which scene_off[B] rows are live, lens = [P] * B.  `points`
    is a list of 1 .. B tensors [n <= P, F] (fewer than B: padded with copies of scene 0, which the gate empties again) or the dict a
    DevicePipeline returns (exactly B scenes; loaded by u3d_batch_ingest, no host read).  The strided sparse levels are sized by
    capture() from sample batches; static shapes are switched on only inside the step's own forward, so `inf.simple_test*` keep
    running exact-size next to it.

    Validity: one device flag = levels over their capacity (native.capacity_flag) + the several-workgroup FPS time-out + scenes the
    ingest cut to P.  u3d_det_gate turns it into `valid` and empties every scene of an invalid replay, so nothing wrong can be read by
    mistake.  Nothing is truncated silently and nothing is re-captured automatically: results() re-runs an invalid batch eagerly and
    counts it in `fallbacks`; capture() may be called again with that batch among the samples.

    Test-time augmentation: InferenceStep(inf, batch_size=B, point_capacity=P, views=A, tta_nms_thr=0.1,
    tta_max_num=500) captures the forward over B * A scenes (scene-major, view-minor), the batched tail into `view_det` [B * A, K, D] and
    the multi-view merge over that padded layout (native.tta_merge_padded) into `det` [B, tta_max_num, D]; the gate, `n_live`,
    `fallbacks` and results() count SAMPLES.  `points` is then the expanded dict a DevicePipeline with MultiScaleFlipAug3D returns (B * A
    scenes, tta_views == A; its tta_params go into the step's static view table with a device-to-device copy) or a list of n * A
    tensors, 1 <= n <= B, with tta_params= f32 [n * A, 9] (missing samples: copies of sample 0's views and table rows, gated away).
    The coordinate code of the merge (Depth / LiDAR) comes from box_type_3d= or from the first dict bound before capture and is fixed
    from then on: a later dict that disagrees is refused.  An invalid replay is re-run through inf.aug_test_batched.  views=1 is the
    step described above, with no view buffers and no further launches.

    Dynamic voxelization (ScanNet-large: dynamic_voxelization=True with a DynamicSimpleVFE): the voxel list is a
    level like the others - capture() sizes it from the same sample forwards (never above B * views * P rows) and returns its size in
    front of `caps`, a list that overflows raises the same flag -, the spare rows of `cat` never become points (u3d_voxelize_dynamic)
    and the voxel means are order-free inside inf.scope() (u3d_scatter_mean_exact), so a replay and its eager fallback agree.

    Limits: an InferenceModel on one device, B and `views` fixed per step, all views of a sample in one batch.  An empty live scene
    gives NaN queries."""

    def __init__(self, inf, batch_size, point_capacity, views=1, tta_nms_thr=0.1, tta_max_num=500, box_type_3d=None):
        A = int(views)
        if A < 1:
            raise ValueError(f"InferenceStep(views={views}): at least one view per sample")
        if not isinstance(inf, InferenceModel):
            raise TypeError(f"InferenceStep captures an InferenceModel, not {type(inf).__name__}: wrap the model first")
        model = inf.model
        from .plugin.detector import DynamicSimpleVFE
        self.dynamic = bool(getattr(model, "dynamic_voxelization", False))
        if self.dynamic and not isinstance(getattr(model, "pts_voxel_encoder", None), DynamicSimpleVFE):
            raise NotImplementedError("InferenceStep: this model has dynamic_voxelization=True and no DynamicSimpleVFE as its voxel encoder - "
                                      "the capacity-sized voxel list of the dynamic route is that encoder's")
        B, P = int(batch_size), int(point_capacity)
        if B < 1:
            raise ValueError(f"InferenceStep(batch_size={batch_size}): at least one scene")
        if P < 1:
            raise ValueError(f"InferenceStep(point_capacity={point_capacity}): at least one point per scene")
        self.inf, self.model = inf, model
        self.batch_size, self.point_capacity = B, P
        self.views, self.tta_nms_thr, self.tta_max_num = A, float(tta_nms_thr), int(tta_max_num)
        if A > 1 and not 1 <= self.tta_max_num <= nv.DET_TAIL_MAX_K:
            raise ValueError(f"InferenceStep(tta_max_num={tta_max_num}): 1 .. {nv.DET_TAIL_MAX_K}")
        self.box_type_3d = box_type_3d
        self.coord = None if box_type_3d is None else _coord_of(box_type_3d)        # views > 1: the merge's coordinate code
        # columns of a point row: the hard VFE names them; DynamicSimpleVFE averages whatever the middle encoder takes
        self.feat = int(model.pts_middle_encoder.in_channels if self.dynamic else model.pts_voxel_encoder.num_features)
        self._vox_cap = None                                      # dynamic voxelization: rows of the voxel list, sized by capture()
        self.fallbacks = 0
        self.pts = self.valid = self.det = self.head_outs = None
        self.view_det = self.tta_params = None                    # views > 1 only: the per-view tail of a replay, the static view table
        self._graph = self._caps = None

    @property
    def n_live(self):
        """Device int32 [1]: the leading scenes of the bound batch that carry real data (the rest is padding the gate empties); None
        before the first batch is bound.  What det_store.DetStore.append takes next to `det` and `valid`."""
        return None if self.pts is None else self._n_live

    # ---- static buffers ---------------------------------------------------------------------------------------------------
    def _alloc(self):
        """The point buffers without GT, this step's flag, FPS time-out record and `valid`.  Allocated once: a graph keeps these addresses."""
        dev = next(self.model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("InferenceStep: the model is not on a GPU")
        self.dev = dev
        self._buf = sb.StaticBatch(self.batch_size * self.views, self.point_capacity, self.feat, dev)
        self.pts = self._buf.pts
        self._n_live = torch.full((1,), self.batch_size, dtype=torch.int32, device=dev)
        self._flag = torch.zeros(1, dtype=torch.float32, device=dev)
        self._fps_err = nv.fps_err_buffer(dev)
        self.valid = torch.zeros(1, dtype=torch.int32, device=dev)
        if self.views > 1:
            self.tta_params = torch.zeros((self.batch_size * self.views, nv.AUG_NPARAM), dtype=torch.float32, device=dev)

    def _view_table(self, tab, rows):
        """The host's checks of a view table of `rows` views: nothing is read."""
        if not torch.is_tensor(tab) or tab.dtype != torch.float32 or tuple(tab.shape) != (rows, nv.AUG_NPARAM):
            raise ValueError(f"InferenceStep: tta_params must be a float32 tensor [{rows}, {nv.AUG_NPARAM}] (one row per view)")
        if tab.device != self.dev:
            raise ValueError(f"InferenceStep: tta_params must live on {self.dev}")
        return tab

    def _bind(self, points, tta_params=None):
        """Load a batch into the static buffers on the current stream -> the number of live samples."""
        if self.pts is None:
            self._alloc()
        B, A = self.batch_size, self.views
        if isinstance(points, dict):
            if A > 1:
                if int(points.get("tta_views", 1)) != A:
                    raise ValueError(f"InferenceStep: the batch has tta_views = {points.get('tta_views', 1)}, the step was built for {A} views")
                off = points.get("scene_off")
                if torch.is_tensor(off) and off.numel() != B * A + 1:
                    raise ValueError(f"InferenceStep: {off.numel() - 1} scenes, the step was built for {B} samples of {A} views")
                tab = self._view_table(points.get("tta_params") if tta_params is None else tta_params, B * A)
                coord = _coord_of(points.get("box_type_3d", "Depth"))
                if self.coord is None and self._graph is None:
                    self.coord, self.box_type_3d = coord, points.get("box_type_3d", "Depth")
                if coord != self.coord:
                    raise ValueError(f"InferenceStep: the batch is in {points.get('box_type_3d', 'Depth')!r} coordinates, the step merges "
                                     f"its views in {self.box_type_3d!r} coordinates")
            self._buf.bind_packed(points, "InferenceStep:")
            if A > 1:
                self.tta_params.copy_(tab)
            n = B
        else:
            points = list(points)
            n, rest = divmod(len(points), A)
            if rest or not 1 <= n <= B:
                raise ValueError(f"InferenceStep: {len(points)} scenes, the step was built for 1 .. {B} samples" + (f" of {A} views" if A > 1 else ""))
            if A > 1:
                if tta_params is None:
                    raise ValueError("InferenceStep: a list of views needs tta_params= (one row per view)")
                tab = self._view_table(tta_params, n * A)
            self._buf.bind_scenes(self.model, points + points[:A] * (B - n), "InferenceStep:")      # the last batch of a dataset: padded, gated away again
            if A > 1:
                self.tta_params[:n * A].copy_(tab)
                if n < B:
                    self.tta_params[n * A:].copy_(tab[:A].repeat(B - n, 1))
        self._n_live.fill_(n)
        return n

    # ---- the forward (same code eager or captured) ----------------------------------------------------------------------------
    @contextlib.contextmanager
    def _static(self):
        """Capacity-sized levels, device-side counts and this step's FPS time-out record - for the step's own forward only."""
        m, enc = self.model, self.model.pts_middle_encoder
        prev = m.static_shapes, enc.level_capacities, m.fps_err
        m.static_shapes, enc.level_capacities, m.fps_err = True, self._caps, self._fps_err
        vfe = m.pts_voxel_encoder if self.dynamic else None
        if vfe is not None:             # dynamic voxelization: the voxel list capacity-sized too, its count left on the device
            prev_vfe = vfe.capacity, vfe.static_eval
            vfe.capacity, vfe.static_eval = self._vox_cap, True
        try:
            yield
        finally:
            m.static_shapes, enc.level_capacities, m.fps_err = prev
            if vfe is not None:
                vfe.capacity, vfe.static_eval = prev_vfe

    @torch.no_grad()
    def _forward(self):
        """A straight line on one stream (extract_pts_feat would fork the FPS onto a side stream: parallel branches in a graph)."""
        m = self.model
        with self.inf.scope(), self._static():
            v = m.stage_voxelize(self.pts)
            fps = m.stage_fps(v)
            feat = m.stage_features(v)
            self.head_outs = m.pts_bbox_head(feat, None, fps)
            self.det = m.pts_bbox_head.get_bboxes_batched(self.head_outs, None)
            if self.views > 1:
                # the views of every sample merged where the tail left them: padded rows, device counts (u3d_tta_merge_padded)
                if self.coord is None:
                    raise RuntimeError("InferenceStep(views > 1): no coordinate code yet - pass box_type_3d= or capture from a packed dict")
                self.view_det = self.det
                self.det = nv.tta_merge_padded(self.view_det, self.tta_params, self.views, self.coord, m.pts_bbox_head.num_classes,
                                               self.tta_nms_thr, self.tta_max_num)
            # the largest set the FPS can see: P points, or the hard voxelizer's limit (dynamic: its voxel-coordinate FPS runs over the
            # per-point rows, and max_voxels is -1)
            times_out = sb.fps_can_time_out(m, self.point_capacity if self.dynamic
                                            else max(self.point_capacity, int(m.pts_voxel_layer.max_voxels[1])))
            sb.validity_flag(m, self._caps, self._fps_err if times_out else None, self._buf.ingest_flag, self._flag)
            nv.det_gate(self.det, self._flag, self._n_live, self.valid)
            self.det.valid = self.valid

    def _drop_outputs(self):
        """Drop every reference to an eager iteration's outputs BEFORE capturing (static_batch.drop_decoder_outputs says why)."""
        self.det = self.view_det = self.head_outs = None
        self.model.pts_middle_encoder.last_level_counts = []
        if self.dynamic:
            self.model.pts_voxel_encoder.last_count_dev = None
        sb.drop_decoder_outputs(self.model)

    def capture(self, batches, margin=1.25, warmup=3):
        """Size the strided sparse levels from exact-size eager forwards over `batches` (each what run() takes - with views > 1 the
        expanded dict or a pair (list of n * A views, tta_params); the largest count per level x margin, rounded up to a multiple of
        256 - static_batch.level_capacity), warm up, capture.  -> (counts, caps).  May be called again, e.g. with a batch that overflowed
        added: the previous graph is dropped."""
        batches = list(batches)
        if not batches:
            raise ValueError("InferenceStep.capture: at least one sample batch")
        if int(warmup) < 1:
            raise ValueError("InferenceStep.capture: at least one warm-up iteration (one-time initialisation must not fall into the capture)")
        self._graph = None
        if self.pts is not None:
            self._drop_outputs()
        enc = self.model.pts_middle_encoder
        seen = []
        for b in batches:
            self._bind(*self._sample(b))
            off = self.pts["scene_off"].tolist()
            exact = dict(cat=self.pts["cat"][:off[-1]], scene_off=self.pts["scene_off"], lens=[off[i + 1] - off[i] for i in range(len(off) - 1)])
            with torch.no_grad(), self.inf.scope():       # the counts come from the encoder: no FPS, no head
                self.model.stage_features(self.model.stage_voxelize(exact))
            seen.append([int(c.item()) for c in enc.last_level_counts])
        counts = sb.max_level_counts(seen)
        self._caps = [sb.level_capacity(c, margin) for c in counts[1:]]
        if self.dynamic:
            # the voxel list (level 0) the same way; every voxel holds a point, so B * views * P rows always suffice
            self._vox_cap = min(sb.level_capacity(counts[0], margin), self.batch_size * self.views * self.point_capacity)
        s = sb.warm_up(self._forward, warmup)            # static-shape eager warm-up on the capture stream
        self._drop_outputs()
        g = sb.capture_graph(self._forward, s)
        torch.cuda.synchronize()
        self._graph = g
        return counts, ([self._vox_cap] if self.dynamic else []) + list(self._caps)

    # ---- use --------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _sample(batch):
        """A sample batch of capture(): what run() takes, or the pair (list of views, tta_params) -> run()'s arguments."""
        if isinstance(batch, tuple) and len(batch) == 2 and torch.is_tensor(batch[1]) and not torch.is_tensor(batch[0]):
            return batch
        return batch, None

    def run(self, points, tta_params=None):
        """Load `points` and replay: -> the native.DetBatch whose tensors are the graph's static outputs (`det.valid` is `step.valid`,
        device int32 [1]: 1 = read it, 0 = every scene was emptied).  THE NEXT run() OVERWRITES THEM - copy what must outlive it.  No
        host read, no allocation outside the graph's pool and no synchronisation for a packed dict; a list costs the host-sized copy of
        pack_points.  `step.head_outs` are the head's raw outputs of the same replay.  views > 1: `det` holds one merged scene per
        sample, `step.view_det` the per-view tail of the same replay; a list of views comes with tta_params= (one row per view)."""
        if self._graph is None:
            raise RuntimeError("InferenceStep.run: capture() first")
        self._bind(points, tta_params)
        self._graph.replay()
        return self.det

    def results(self, points, img_metas=None, tta_params=None):
        """run() and the one read of the tail (and of `valid` with it) -> simple_test_batched's list of dicts on the host, one per
        live sample.  An invalid replay is re-run through inf.simple_test_batched - with views > 1 through inf.aug_test_batched -
        (eager, exact-size) and counted in `fallbacks`."""
        det = self.run(points, tta_params)
        n = self.batch_size if isinstance(points, dict) else len(points) // self.views
        host, valid = det.cpu(), int(self.valid.cpu()[0])
        if valid:
            return [dict(boxes_3d=b, scores_3d=s, labels_3d=l) for b, s, l in host.to_list()[:n]]
        self.fallbacks += 1
        if self.views > 1:
            return self.inf.aug_test_batched(points if isinstance(points, dict) else list(points), tta_params=tta_params, views=self.views,
                                             box_type_3d=self.box_type_3d, nms_thr=self.tta_nms_thr, max_num=self.tta_max_num)
        if isinstance(points, dict):
            from .datapath import unpack_batch
            points = unpack_batch({k: points[k] for k in ("points", "scene_off", "count") if k in points})[0]
        return self.inf.simple_test_batched(img_metas, list(points))

    def overflows(self):
        """Packed batches the ingest had to cut to point_capacity so far (their replays were invalid).  One small device-to-host read."""
        return 0 if self.pts is None else int(self._buf.ingest_over.sum().item())
