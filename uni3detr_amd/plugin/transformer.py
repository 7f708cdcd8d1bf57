"""Uni3DETRTransformer / Uni3DETRTransformerDecoder / UniCrossAtten behind the reference's registry names
(ref: projects/mmdet3d_plugin/models/utils/uni3detr_transformer.py:18-360) plus the mmcv bricks the shipped configs name
(`BaseTransformerLayer`, `MultiheadAttention`, `FFN`).

Execution differs from the reference on purpose: the reference loops over query groups and runs the 3-layer decoder
once per group; groups never interact, so here all groups of all scenes run together — every linear layer sees
[B, groups*nq, C] rows and self-attention is block-diagonal over [B*groups, nq] — with identical results.
Tensors are batch-first internally.  Parameter names are the reference checkpoints' (SURVEY.md Appendix C).
"""
import copy
import math

import torch
import torch.nn.functional as F
from torch import nn

from .. import native as nv
from ..shadow import compute_copy
from ..registry import ATTENTION, FEEDFORWARD_NETWORK, TRANSFORMER, TRANSFORMER_LAYER, TRANSFORMER_LAYER_SEQUENCE
from . import param_grads as PG
from .param_grads import deferred_param_grads, flush_deferred, reset_param_uses  # noqa: F401  (the trainer and the tests reach them here)


def inverse_sigmoid(x, eps=1e-5):
    x = x.clamp(min=0, max=1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


_ONES = {}


def ones_vector(n, device, dtype):
    key = (str(device), int(n), dtype)
    t = _ONES.get(key)
    if t is None:
        t = torch.ones(int(n), device=device, dtype=dtype)
        _ONES[key] = t
    return t


def colsum(x2):
    """Differentiable column sums of a [M, N] matrix as a GEMV with a ones vector.  NOT x2.sum(0): torch's multi-block reduce
    kernel returns garbage for ~30 % of such reductions when replayed from a HIP graph on this stack (tools/reduce_probe.py),
    GEMV does not.  (Inside backward passes the HIP kernel nv.colsum is used instead: rocBLAS gemv takes ~70 us here.)"""
    return torch.mv(x2.t(), ones_vector(x2.shape[0], x2.device, x2.dtype))


def _mm_f32(a, b):
    """a @ b for bf16 operands with an f32 result, in one launch when the BLAS backend supports out_dtype."""
    if MM_OUT_DTYPE[0] is None:
        try:
            torch.mm(a[:1], b, out_dtype=torch.float32)
            MM_OUT_DTYPE[0] = True
        except Exception:                                     # noqa: BLE001 - capability probe
            MM_OUT_DTYPE[0] = False
    if MM_OUT_DTYPE[0]:
        return torch.mm(a, b, out_dtype=torch.float32)
    return (a @ b).float()


MM_OUT_DTYPE = [None]


def _linear_backward(dy2, x2, wc, need_dx, need_dw, need_db, xdtype, wid, kind="linear", r0=0, dw_out=None, db_out=None):
    """Shared backward of y = x2 @ wc^T + b.  dy2 [M,N], x2 [M,K], wc [N,K] (compute dtype) = rows r0.. of the weight noted as
    `wid`.  Parameter gradients come back in f32, in dw_out / db_out when given (dW from the HIP row-split wgrad kernel when bf16:
    hipBLASLt runs these [N,M]x[M,K] products with M = B*900 on 16 tiles; db from u3d_colsum — NOT dy.sum(0), see colsum), from
    where param_grads.layer_route says; a queued one is an unwritten placeholder."""
    (n, k), m, bf16 = wc.shape, x2.shape[0], wc.dtype == torch.bfloat16
    dx = dw = db = None
    if need_dx:
        dx = _mm_f32(dy2, wc) if (bf16 and xdtype == torch.float32) else (dy2 @ wc).to(xdtype)
    # a graph built before the last reset_param_uses() finds nothing under its `wid`: never single, nothing queued
    weight, bias = PG.USES.params.get(wid, (None, None))
    q = PG.QUEUE
    r = PG.layer_route(kind, q is not None, PG.USES.single(weight), need_dw, need_db, bf16, m, n, k, has_bias=bias is not None,
                       on_gpu=dy2.is_cuda, own_wgrad=OWN_WGRAD, skinny_wgrad=SKINNY_WGRAD)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dy2.device)      # noqa: E731
    if r.dw == "queue":
        q.product(dy2, x2.contiguous(), weight, bias if r.db else None, r0, r0 + n)
        dw = dw_out if dw_out is not None else new(n, k)
    elif r.dw in ("partial", "partial_queue"):
        partial = nv.skinny_wgrad_partial(dy2, x2.contiguous())
        dw = nv.colsum(partial).view(n, k) if r.dw == "partial" else new(n, k)
        if r.dw == "partial_queue":
            q.colsum(partial, weight)
    elif r.dw == "own":
        dw = nv.spconv_wgrad(dy2, x2.contiguous(), None, nv.count_tensor(m, dy2.device), 1).view(n, k)
    elif r.dw == "blas":
        dw = _mm_f32(dy2.t(), x2) if bf16 else dy2.t() @ x2
    if r.dw in ("own", "blas") and dw_out is not None:
        dw = dw_out.copy_(dw)
    if r.db in ("queue", "sum_queue"):
        db = db_out if db_out is not None else new(n)
        if r.db == "sum_queue":
            q.colsum(dy2, bias)
    elif r.db == "sum":
        db = nv.colsum(dy2) if db_out is None else db_out.copy_(nv.colsum(dy2))
    return dx, dw, db


class _TorchLinearFn(torch.autograd.Function):
    """F.linear on the fp32 master parameters, computed in `cdt` (None = as is): the low-precision weight comes from the
    per-step shadow set (uni3detr_amd/shadow.py), the backward is graph-replay-safe and returns f32 parameter gradients."""

    @staticmethod
    def forward(ctx, x, weight, bias, cdt, relu=False):
        if cdt is not None:
            xc = x if x.dtype == cdt else x.to(cdt)
            wc, bc = compute_copy(weight, cdt), compute_copy(bias, cdt)
        else:
            xc, wc, bc = x, weight, bias
        ctx.has_bias, ctx.xdtype = bias is not None, x.dtype
        ctx.wid = PG.USES.note(weight, bias)
        ctx.relu = relu
        if relu:
            if bc is not None and xc.dim() >= 2 and bc.dtype == xc.dtype == wc.dtype:
                # bias + ReLU in the GEMM epilogue (hipBLASLt), not a separate pass over the output
                y = torch._addmm_activation(bc, xc.reshape(-1, xc.shape[-1]), wc.t(), use_gelu=False).view(*xc.shape[:-1], wc.shape[0])
            else:
                y = F.linear(xc, wc, bc).relu_()
            ctx.save_for_backward(xc, wc, y)
            return y
        ctx.save_for_backward(xc, wc)
        return F.linear(xc, wc, bc)

    @staticmethod
    def backward(ctx, dy):
        if ctx.relu:
            xc, wc, y = ctx.saved_tensors
            dy = torch.ops.aten.threshold_backward(dy.contiguous() if dy.dtype == y.dtype else dy.to(y.dtype), y, 0)
        else:
            xc, wc = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        dy2 = (dy2 if dy2.dtype == wc.dtype else dy2.to(wc.dtype)).contiguous()
        x2 = xc.reshape(-1, xc.shape[-1])
        need_db = ctx.has_bias and ctx.needs_input_grad[2]
        dx, dw, db = _linear_backward(dy2, x2, wc, ctx.needs_input_grad[0], ctx.needs_input_grad[1], need_db, ctx.xdtype, ctx.wid)
        return (None if dx is None else dx.view(xc.shape)), dw, db, None, None


class _InProjFn(torch.autograd.Function):
    """nn.MultiheadAttention's packed in-projection with q = k input `qk` and value input `xv`:
    (qk @ W[:2C]^T + b[:2C],  xv @ W[2C:]^T + b[2C:]) with ONE gradient for the packed parameter."""

    @staticmethod
    def forward(ctx, qk, xv, weight, bias, cdt):
        c = weight.shape[1]
        if cdt is not None:
            qc = qk if qk.dtype == cdt else qk.to(cdt)
            vc = xv if xv.dtype == cdt else xv.to(cdt)
            wc, bc = compute_copy(weight, cdt), compute_copy(bias, cdt)
        else:
            qc, vc, wc, bc = qk, xv, weight, bias
        ctx.save_for_backward(qc, vc, wc)
        ctx.qdtype, ctx.vdtype = qk.dtype, xv.dtype
        ctx.wid = PG.USES.note(weight, bias)
        return F.linear(qc, wc[: 2 * c], bc[: 2 * c]), F.linear(vc, wc[2 * c:], bc[2 * c:])

    @staticmethod
    def backward(ctx, dqk, dv):
        qc, vc, wc = ctx.saved_tensors
        c = wc.shape[1]
        cast = lambda t: (t if t.dtype == wc.dtype else t.to(wc.dtype)).reshape(-1, t.shape[-1]).contiguous()
        dqk2, dv2 = cast(dqk), cast(dv)
        need_w, need_b = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        dw = torch.empty((3 * c, c), dtype=torch.float32, device=dqk2.device) if need_w else None
        db = torch.empty((3 * c,), dtype=torch.float32, device=dqk2.device) if need_w else None
        dq_in, _, _ = _linear_backward(dqk2, qc.reshape(-1, c), wc[: 2 * c], ctx.needs_input_grad[0], need_w, need_b, ctx.qdtype,
                                       ctx.wid, "inproj", 0, None if dw is None else dw[: 2 * c], None if db is None else db[: 2 * c])
        dv_in, _, _ = _linear_backward(dv2, vc.reshape(-1, c), wc[2 * c:], ctx.needs_input_grad[1], need_w, need_b, ctx.vdtype,
                                       ctx.wid, "inproj", 2 * c, None if dw is None else dw[2 * c:], None if db is None else db[2 * c:])
        return (None if dq_in is None else dq_in.view(qc.shape)), (None if dv_in is None else dv_in.view(vc.shape)), dw, db, None


SAFE_LINEAR = True        # test-only module attribute (tests/test_toggles_gpu.py): False restores torch's own Linear backward
OWN_WGRAD = True          # dW of the decoder/head linears on u3d_igemm_wgrad_bf16
# dW of the <= 16-feature linears on u3d_skinny_wgrad_bf16: correct (tests) but measured SLOWER end to end than hipBLASLt's
# small products (30.3 vs 29.7 ms per step: 57 workgroups per launch) - opt-in until the kernel splits the wide dimension too
RELU_EPILOGUE = True   # Linear+ReLU: activation in the GEMM epilogue (torch._addmm_activation)
SKINNY_WGRAD = False
# The layer-by-layer formulation of the decoder further down (nn.Linear / SDPA through ATen) is what runs on CPU tensors (the
# registry / config tests of this container) and what the GPU tests compare the fused HIP decoder with by setting
# fused_decoder.ENABLED = False themselves.  No environment variable selects it: on a CUDA tensor a call the fused kernels do not cover
# raises (Uni3DETRTransformerDecoder._fused_decoder).


def _autocast_dtype(x):
    return torch.get_autocast_dtype('cuda') if (x.is_cuda and torch.is_autocast_enabled()) else None


def fast_linear(x, lin, relu=False, weight=None, bias=None):
    """nn.Linear `lin` (or explicit weight/bias) applied to x; HIP GEMM with fused bias/ReLU when running in bf16 mode."""
    w = lin.weight if weight is None else weight
    b = (lin.bias if lin is not None else None) if bias is None and weight is None else bias
    if SAFE_LINEAR and x.is_cuda and torch.is_grad_enabled() and (x.requires_grad or w.requires_grad):
        if relu and RELU_EPILOGUE:
            return _TorchLinearFn.apply(x, w, b, _autocast_dtype(x), True)
        y = _TorchLinearFn.apply(x, w, b, _autocast_dtype(x))
    else:
        y = F.linear(x, w, b)
    return F.relu(y) if relu else y


class _FusedLN(torch.autograd.Function):
    """nn.LayerNorm (+ ReLU) on the HIP row kernels: one launch forward, one backward; the output can be produced directly in the
    compute dtype of the GEMM that follows; dgamma / dbeta are deferred and batched like the linear parameter gradients."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, relu, out_dtype):
        shp = x.shape
        x2 = x.reshape(-1, shp[-1])
        x2 = x2 if x2.is_contiguous() else x2.contiguous()
        y, mean, rstd = nv.layernorm_fwd(x2, weight, bias, eps, relu, out_dtype)
        ctx.save_for_backward(x2, weight, bias, mean, rstd)
        ctx.relu, ctx.shp = relu, shp
        PG.USES.note(weight, bias)
        return y.view(shp)

    @staticmethod
    def backward(ctx, dy):
        x2, weight, bias, mean, rstd = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        dy2 = dy2 if dy2.is_contiguous() else dy2.contiguous()
        dx, partial = nv.layernorm_bwd(dy2, x2, weight, bias, mean, rstd, ctx.relu)
        q = PG.QUEUE
        r = PG.layer_route("norm", q is not None, PG.USES.single(weight), ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        if r.dw == "sum_queue":
            q.colsum(partial[0], weight)
            q.colsum(partial[1], bias)
            dg, db = (torch.empty((x2.shape[1],), dtype=torch.float32, device=x2.device) for _ in "gb")     # written by the flush
        else:
            dg, db = nv.colsum(partial[0]), nv.colsum(partial[1])
        return dx.view(ctx.shp), dg, db, None, None, None


FUSED_LN = True
SHARED_VALUE_GRAD = True


def fused_layer_norm(x, ln, relu=False, out_dtype=None):
    """`ln` (nn.LayerNorm over the last dim) applied to x, optionally followed by ReLU, on the HIP kernels when x is on the GPU."""
    if (FUSED_LN and x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and ln.elementwise_affine and ln.bias is not None
            and len(ln.normalized_shape) == 1 and x.shape[-1] == ln.normalized_shape[0] and x.shape[-1] <= 1024 and x.numel() > 0
            and ln.weight.dtype == torch.float32):
        return _FusedLN.apply(x, ln.weight, ln.bias, ln.eps, relu, out_dtype or x.dtype)
    y = ln(x)
    y = F.relu(y) if relu else y
    return y if out_dtype is None else y.to(out_dtype)


def residual_add(x, o):
    """x + o with o brought to x's dtype first (see MultiheadAttention.forward_grouped on mixed-dtype adds)."""
    return x + (o if o.dtype == x.dtype else o.to(x.dtype))


def run_sequential(seq, x):
    """nn.Sequential of Linear / LayerNorm / ReLU / Dropout (the head branches, position encoder, FFN) with Linear(+ReLU)
    routed through fast_linear."""
    mods = list(seq)
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.LayerNorm):
            fuse = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
            nxt = mods[i + (2 if fuse else 1)] if i + (2 if fuse else 1) < len(mods) else None
            cdt = _autocast_dtype(x)
            # a Linear right behind it takes the compute dtype straight from the norm kernel (no cast launch)
            x = fused_layer_norm(x, m, relu=fuse, out_dtype=cdt if (cdt is not None and isinstance(nxt, nn.Linear)) else None)
            i += 2 if fuse else 1
        elif isinstance(m, nn.Linear):
            fuse = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
            x = fast_linear(x, m, relu=fuse)
            i += 2 if fuse else 1
        elif isinstance(m, nn.Sequential):
            x = run_sequential(m, x)
            i += 1
        else:
            x = m(x)
            i += 1
    return x


class MLP(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, num_layers):
        super().__init__()
        self.num_layers = num_layers
        dims = [input_dim] + [hidden_dim] * (num_layers - 1) + [output_dim]
        self.layers = nn.ModuleList(nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:]))

    def forward(self, x):
        for i, l in enumerate(self.layers):
            x = fast_linear(x, l, relu=i < self.num_layers - 1)
        return x


_SINE_CACHE = {}


def get_sine_pos_embed(pos, num_pos_feats=128, temperature=10000, exchange_xy=False):
    """pos [..., n] in [0,1] -> [..., n*num_pos_feats]: interleaved sin/cos of pos*2pi/T^(2*(i//2)/F) (ref :33-65)."""
    key = (pos.device, num_pos_feats, temperature)
    dim_t = _SINE_CACHE.get(key)
    if dim_t is None:
        d = torch.arange(num_pos_feats, dtype=torch.float32, device=pos.device)
        dim_t = temperature ** (2 * torch.div(d, 2, rounding_mode="floor") / num_pos_feats)
        _SINE_CACHE[key] = dim_t
    s = pos.float().unsqueeze(-1) * (2 * math.pi) / dim_t                      # [..., n, F]
    emb = torch.stack((s[..., 0::2].sin(), s[..., 1::2].cos()), dim=-1).flatten(-2)
    if exchange_xy:
        emb = torch.cat([emb[..., 1:2, :], emb[..., 0:1, :], emb[..., 2:, :]], dim=-2)
    return emb.flatten(-2)


class _SineEmbed(torch.autograd.Function):
    """get_sine_pos_embed(ref_logits.sigmoid()) in the dtype the consumer wants: one HIP launch each way (u3d_sine_embed_fwd/_bwd)."""

    @staticmethod
    def forward(ctx, ref_logits, dim_t, out_dtype):
        l2 = ref_logits.reshape(-1, ref_logits.shape[-1]).contiguous().float()
        ctx.save_for_backward(l2, dim_t)
        ctx.shape, ctx.in_dtype = ref_logits.shape, ref_logits.dtype
        return nv.sine_embed_fwd(l2, dim_t, out_dtype).view(*ref_logits.shape[:-1], -1)

    @staticmethod
    def backward(ctx, dout):
        l2, dim_t = ctx.saved_tensors
        d2 = dout.reshape(l2.shape[0], -1)
        d2 = d2 if (d2.is_contiguous() and d2.dtype in (torch.float32, torch.bfloat16)) else d2.contiguous().float()
        return nv.sine_embed_bwd(l2, dim_t, d2).view(ctx.shape).to(ctx.in_dtype), None, None


FUSED_SINE_EMBED = True


def sine_embed_of_logits(ref_logits, out_dtype, num_pos_feats=128, temperature=10000):
    """get_sine_pos_embed(ref_logits.sigmoid()).to(out_dtype) (ref :181), fused on the GPU."""
    if FUSED_SINE_EMBED and ref_logits.is_cuda and out_dtype in (torch.float32, torch.bfloat16):
        key = (ref_logits.device, num_pos_feats, temperature)
        dim_t = _SINE_CACHE.get(key)
        if dim_t is None:
            d = torch.arange(num_pos_feats, dtype=torch.float32, device=ref_logits.device)
            dim_t = temperature ** (2 * torch.div(d, 2, rounding_mode="floor") / num_pos_feats)
            _SINE_CACHE[key] = dim_t
        return _SineEmbed.apply(ref_logits, dim_t, out_dtype)
    return get_sine_pos_embed(ref_logits.sigmoid(), num_pos_feats, temperature).to(out_dtype)


@ATTENTION.register_module()
class MultiheadAttention(nn.Module):
    """mmcv wrapper semantics: q = k = query + query_pos, v = query, residual + dropout (legacy `dropout=` sets both the
    attention dropout and the residual dropout)."""

    def __init__(self, embed_dims, num_heads, attn_drop=0.0, proj_drop=0.0, dropout_layer=None, init_cfg=None,
                 batch_first=False, dropout=None, **kwargs):
        super().__init__()
        if dropout is not None:
            attn_drop = dropout
            dropout_layer = dict(type="Dropout", drop_prob=dropout)
        self.embed_dims, self.num_heads, self.batch_first = embed_dims, num_heads, batch_first
        self.attn = nn.MultiheadAttention(embed_dims, num_heads, attn_drop)
        self.attn_drop = attn_drop
        self.proj_drop = nn.Dropout(proj_drop)
        self.dropout_layer = nn.Dropout(dropout_layer["drop_prob"]) if dropout_layer else nn.Identity()

    def forward_grouped(self, x, pos, group, x_c=None):
        """x, pos: [B, G*group, C]; attention within each group of `group` queries.  x_c: x already in the compute dtype."""
        B, N, C = x.shape
        H = self.num_heads
        cdt = _autocast_dtype(x)
        if cdt is not None and x.dtype != cdt:
            # one cast of the f32 stream serves q = k and v; a mixed f32 + bf16 add runs on torch's "templated" kernel at ~40 us
            # for [8,900,256] (a same-dtype add: 4 us), so every mixed add of the layer is written as cast + add
            xb = x_c if x_c is not None else x.to(cdt)
            qk = (xb + pos.to(cdt)).reshape(-1, group, C)
            xv = xb.reshape(-1, group, C)
        else:
            qk = (x + pos).reshape(-1, group, C)
            xv = x.reshape(-1, group, C)
        w, b = self.attn.in_proj_weight, self.attn.in_proj_bias
        if SAFE_LINEAR and x.is_cuda and torch.is_grad_enabled() and b is not None:
            qk_p, v = _InProjFn.apply(qk, xv, w, b, _autocast_dtype(x))
        else:
            qk_p = fast_linear(qk, None, weight=w[: 2 * C], bias=b[: 2 * C])
            v = fast_linear(xv, None, weight=w[2 * C:], bias=b[2 * C:])
        q, k = qk_p[..., :C], qk_p[..., C:]
        sh = lambda t: t.reshape(-1, group, H, C // H).transpose(1, 2)
        o = F.scaled_dot_product_attention(sh(q), sh(k), sh(v), dropout_p=self.attn_drop if self.training else 0.0)
        o = o.transpose(1, 2).reshape(B, N, C)
        o = fast_linear(o, self.attn.out_proj)
        return residual_add(x, self.dropout_layer(self.proj_drop(o)))


@FEEDFORWARD_NETWORK.register_module()
class FFN(nn.Module):
    def __init__(self, embed_dims=256, feedforward_channels=1024, num_fcs=2, act_cfg=dict(type="ReLU", inplace=True),
                 ffn_drop=0.0, dropout_layer=None, add_identity=True, init_cfg=None, **kwargs):
        super().__init__()
        layers, c = [], embed_dims
        for _ in range(num_fcs - 1):
            layers.append(nn.Sequential(nn.Linear(c, feedforward_channels), nn.ReLU(inplace=True), nn.Dropout(ffn_drop)))
            c = feedforward_channels
        layers += [nn.Linear(feedforward_channels, embed_dims), nn.Dropout(ffn_drop)]
        self.layers = nn.Sequential(*layers)
        self.dropout_layer = nn.Dropout(dropout_layer["drop_prob"]) if dropout_layer else nn.Identity()
        self.add_identity = add_identity

    def forward(self, x, identity=None):
        out = self.dropout_layer(run_sequential(self.layers, x))
        if not self.add_identity:
            return out
        return residual_add(x if identity is None else identity, out)


class ValueGradAccum:
    """Shared f32 accumulator for the gradient of ONE voxel volume sampled by several decoder layers: every layer's backward adds
    into the same buffer and only the last one to run hands the sum (cast once) to autograd - instead of a zero-fill, a cast and a
    gradient-accumulation add of the whole [B*D*H*W, C] volume per layer."""

    def __init__(self, uses):
        self.uses = self.remaining = uses
        self.buf = None
        self.records = None       # fused decoder, bf16: the layers' value-gradient records, scattered together by the last backward


class _TrilinearSample(torch.autograd.Function):
    """F.grid_sample(value [B,C,D,H,W], grid [B,1,1,N,3]) -> [B,N,C] on the HIP sampler (channels-last rows)."""

    @staticmethod
    def forward(ctx, value, grid, accum=None):
        B, C, D, H, W = value.shape
        rows = value.permute(0, 2, 3, 4, 1).reshape(-1, C)      # no copy for channels_last_3d volumes
        rows = rows if rows.is_contiguous() else rows.contiguous()
        g = grid.float().contiguous()
        ctx.save_for_backward(rows, g)
        ctx.shape = (B, C, D, H, W)
        ctx.accum = accum
        return nv.trilinear_fwd(rows, g, B, (D, H, W))

    @staticmethod
    def backward(ctx, dout):
        rows, g = ctx.saved_tensors
        B, C, D, H, W = ctx.shape
        acc = ctx.accum
        want_dv = ctx.needs_input_grad[0]
        if acc is None or not want_dv:
            dv, dg = nv.trilinear_bwd(rows, g, dout.contiguous().to(rows.dtype), B, (D, H, W), want_dv, ctx.needs_input_grad[1])
            if dv is not None:
                dv = dv.to(rows.dtype).view(B, D, H, W, C).permute(0, 4, 1, 2, 3)
            return dv, dg, None
        if acc.buf is None:
            acc.buf = torch.zeros(rows.shape, dtype=torch.float32, device=rows.device)
        _, dg = nv.trilinear_bwd(rows, g, dout.contiguous().to(rows.dtype), B, (D, H, W), True, ctx.needs_input_grad[1], dvalue_accum=acc.buf)
        acc.remaining -= 1
        dv = None
        if acc.remaining == 0:
            dv = acc.buf.to(rows.dtype).view(B, D, H, W, C).permute(0, 4, 1, 2, 3)
            acc.buf = None
        return dv, dg, None


@ATTENTION.register_module()
class UniCrossAtten(nn.Module):
    """One trilinear sample of the voxel volume per query, gated by sigmoid(Linear(query+pos)), projected, plus the
    residual and an encoding of the reference-point logits (ref :216-360)."""

    def __init__(self, embed_dims=256, num_heads=8, num_points=1, num_sweeps=1, cam_sweep_feq=12, voxel_range=(0, 0, 0),
                 im2col_step=64, dropout=0.1, norm_cfg=None, init_cfg=None, batch_first=False, fp16_enabled=False):
        super().__init__()
        if embed_dims % num_heads != 0:
            raise ValueError(f"embed_dims must be divisible by num_heads, but got {embed_dims} and {num_heads}")
        self.embed_dims, self.num_heads, self.num_points, self.num_sweeps = embed_dims, num_heads, num_points, num_sweeps
        self.dropout = nn.Dropout(dropout)
        self.attention_weights = nn.Linear(embed_dims, num_points)
        self.output_proj = nn.Linear(embed_dims, embed_dims)
        self.position_encoder = nn.Sequential(nn.Linear(3, embed_dims), nn.LayerNorm(embed_dims), nn.ReLU(inplace=True),
                                              nn.Linear(embed_dims, embed_dims), nn.LayerNorm(embed_dims), nn.ReLU(inplace=True))
        self.batch_first = batch_first
        self.init_weight()
        if fp16_enabled:
            self.fp16_enabled = fp16_enabled

    def init_weight(self):
        nn.init.constant_(self.attention_weights.weight, 0.0)
        nn.init.constant_(self.attention_weights.bias, 0.0)
        nn.init.xavier_uniform_(self.output_proj.weight)
        nn.init.constant_(self.output_proj.bias, 0.0)

    def forward_bf(self, query, query_pos, value, ref_logits, accum=None):
        """query/query_pos [B,N,C]; value [B,C,D,H,W] (or [B,C,H,W]); ref_logits [B,N,3] -> [B,N,C]."""
        cdt = _autocast_dtype(query)
        qp = (query.to(cdt) + query_pos.to(cdt)) if (cdt is not None and query.dtype != cdt) else query + query_pos
        w = fast_linear(qp, self.attention_weights).sigmoid()                         # [B,N,P]
        g = (ref_logits.sigmoid() - 0.5) * 2
        B, N, _ = g.shape
        if value.dim() != 5:
            raise NotImplementedError("height-less (BEV) value maps are not used by any shipped Uni3DETR config")
        samp = _TrilinearSample.apply(value, g, accum)                                # [B,N,C]
        wsum = w if w.shape[-1] == 1 else w.sum(-1, keepdim=True)      # num_points = 1 in every shipped config: no reduction launch
        cdt = _autocast_dtype(query)
        if cdt is not None:             # gate in the compute dtype: the product feeds a bf16 GEMM directly
            gated = samp.to(cdt) * wsum.to(cdt)
        else:
            gated = samp.to(query.dtype) * wsum
        out = fast_linear(gated, self.output_proj)
        pos_feat = run_sequential(self.position_encoder, ref_logits.to(query.dtype))
        return residual_add(residual_add(query, self.dropout(out)), pos_feat)


@TRANSFORMER_LAYER.register_module()
class BaseTransformerLayer(nn.Module):
    """(self_attn, norm, cross_attn, norm, ffn, norm) post-norm layer; members `attentions`, `ffns`, `norms`."""

    def __init__(self, attn_cfgs=None, ffn_cfgs=None, operation_order=None, norm_cfg=dict(type="LN"), init_cfg=None,
                 batch_first=False, **kwargs):
        super().__init__()
        self.operation_order = tuple(operation_order)
        n_attn = self.operation_order.count("self_attn") + self.operation_order.count("cross_attn")
        if isinstance(attn_cfgs, dict):
            attn_cfgs = [copy.deepcopy(attn_cfgs) for _ in range(n_attn)]
        assert len(attn_cfgs) == n_attn
        self.attentions = nn.ModuleList(ATTENTION.build(c) for c in attn_cfgs)
        self.embed_dims = self.attentions[0].embed_dims
        n_ffn = self.operation_order.count("ffn")
        if isinstance(ffn_cfgs, dict):
            ffn_cfgs = [copy.deepcopy(ffn_cfgs) for _ in range(n_ffn)]
        self.ffns = nn.ModuleList()
        for c in ffn_cfgs:
            c = dict(c)
            c.setdefault("type", "FFN")
            self.ffns.append(FEEDFORWARD_NETWORK.build(c))
        assert norm_cfg["type"] == "LN"
        self.norms = nn.ModuleList(nn.LayerNorm(self.embed_dims) for _ in range(self.operation_order.count("norm")))
        self.pre_norm = self.operation_order[0] == "norm"
        if self.pre_norm:
            raise NotImplementedError("pre-norm ordering is not used by any shipped Uni3DETR config")

    def forward_bf(self, x, pos, value, ref_logits, group, x_c=None, accum=None):
        ai = ni = fi = 0
        for op in self.operation_order:
            if op == "self_attn":
                x = self.attentions[ai].forward_grouped(x, pos, group, x_c if ai == 0 else None); ai += 1
            elif op == "cross_attn":
                x = self.attentions[ai].forward_bf(x, pos, value, ref_logits, accum); ai += 1
            elif op == "norm":
                x = fused_layer_norm(x, self.norms[ni]); ni += 1
            elif op == "ffn":
                x = self.ffns[fi](x); fi += 1
        return x


@TRANSFORMER_LAYER_SEQUENCE.register_module()
class Uni3DETRTransformerDecoder(nn.Module):
    def __init__(self, transformerlayers=None, num_layers=None, init_cfg=None, return_intermediate=False):
        super().__init__()
        self.num_layers = num_layers
        self.return_intermediate = return_intermediate
        self.layers = nn.ModuleList(TRANSFORMER_LAYER.build(copy.deepcopy(transformerlayers)) for _ in range(num_layers))
        self.embed_dims = self.layers[0].embed_dims
        self.d_model = d = 256
        self.query_scale = MLP(d, d, d, 3)
        self.ref_point_head = MLP(384, d, d, 3)
        self._xyz_cols = None

    def _fused_decoder(self, query, value, reg_branches):
        """The FusedDecoder serving this call, or None (CPU, a layout the fused kernels do not cover)."""
        from . import fused_decoder as _fdm
        hb = getattr(self, "_head_branches", None)
        self._fused_et = _fdm.element_type(self, query, value, reg_branches, hb)
        why = None
        if self._fused_et is None:
            why = "layout / dtype outside the fused kernels (bf16 autocast or plain f32, 256-wide value and queries, per-layer branches)"
        else:
            key = (tuple(id(m) for m in reg_branches), tuple(id(m) for m in hb[0]), tuple(id(m) for m in hb[1]))
            cached = getattr(self, "_fused_cache", None)
            if cached is None or cached[0] != key:
                try:
                    cached = (key, _fdm.FusedDecoder(self, reg_branches, hb[0], hb[1]), None)
                except ValueError as e:
                    cached = (key, None, str(e))
                object.__setattr__(self, "_fused_cache", cached)
            if cached[1] is not None:
                return cached[1]
            why = cached[2]
        # not covered.  On the GPU the layer-by-layer formulation below would run on vendor kernels (F.linear -> hipBLASLt, SDPA): a
        # different product, so the call fails instead - there is no switch a user can set (the tests that compare the two
        # formulations flip fused_decoder.ENABLED in-process)
        if query.is_cuda and _fdm.ENABLED:
            raise RuntimeError(f"Uni3DETRTransformerDecoder: the fused HIP decoder does not cover this call ({why}); there is no vendor-kernel "
                               f"fallback in this package")
        return None

    def forward_bf(self, query, ref_logits, value, reg_branches, group, ref_sig=None):
        """query [B,N,C], ref_logits [B,N,3] -> (states [L,B,N,C], refs [L,B,N,3] logits after each layer's refinement).
        ref_sig: sigmoid(ref_logits) when the caller already has it (the head's fused query assembly)."""
        self._cls_outputs = self._iou_outputs = self._coord_outputs = self._refs_sig = None
        fd = self._fused_decoder(query, value, reg_branches)
        if fd is not None:
            # every layer is one fused HIP call each way (plugin/fused_decoder.py; u3d_decoder_layer_fwd/_bwd): the bf16 instantiation
            # under bf16 autocast (throughput mode), the exact-f32 instantiation of the same kernels for f32 tensors (parity mode)
            from . import fused_decoder as _fdm
            res = _fdm.run(fd, query, ref_logits, value, group, self._fused_et, getattr(self, "_pc_range", None), ref_sig)
            states, refs, regs, clss, ious = res[:5]
            self._reg_outputs, self._cls_outputs, self._iou_outputs, self._states_c = regs, clss, ious, None
            if len(res) > 5:             # the layer tails ran as one launch each: decoded boxes + the stacked reference points came with them
                self._coord_outputs, refs_stacked, self._refs_sig = res[5], res[6], res[7]
                if self.return_intermediate:
                    return torch.stack(states), refs_stacked
                return states[-1], refs[-1]
            if self.return_intermediate:
                return torch.stack(states), torch.stack(refs)
            return states[-1], refs[-1]
        out = query
        states, refs = [], []
        self._reg_outputs = [] if reg_branches is not None else None     # reused by Uni3DETRHead.forward (same module, same input)
        # one gradient accumulator for the sampled volume when every layer samples it exactly once (the shipped layer layout)
        n_cross = sum(l.operation_order.count("cross_attn") for l in self.layers)
        accum = ValueGradAccum(n_cross) if (SHARED_VALUE_GRAD and value.requires_grad and torch.is_grad_enabled() and n_cross > 1) else None
        cdt = _autocast_dtype(query)
        self._states_c = [] if cdt is not None else None      # each layer state once in the compute dtype: shared by the reg branch,
        out_c = None                                          # query_scale, the next layer's self-attention and the head's cls / iou branches
        for lid, layer in enumerate(self.layers):
            raw = self.ref_point_head(sine_embed_of_logits(ref_logits, cdt if cdt is not None else out.dtype))     # the MLP's input dtype: no cast launch
            pos = raw if lid == 0 else self.query_scale(out if out_c is None else out_c) * raw
            out = layer.forward_bf(out, pos, value, ref_logits, group, out_c, accum)
            if cdt is not None:
                out_c = out.to(cdt)
                self._states_c.append(out_c)
            if reg_branches is not None:
                tmp = run_sequential(reg_branches[lid], out if out_c is None else out_c)
                self._reg_outputs.append(tmp)
                assert ref_logits.shape[-1] == 3
                td = tmp.detach()
                if self._xyz_cols is None or self._xyz_cols.device != td.device:
                    self._xyz_cols = torch.tensor([0, 1, 4], device=td.device)
                # (x, y, z) offsets sit in code columns 0, 1, 4 (ref :194-202): one gather + one add instead of three adds + a stack
                ref_logits = (ref_logits.detach() + td.index_select(-1, self._xyz_cols).to(ref_logits.dtype)).detach()
            states.append(out)
            refs.append(ref_logits)
        if self.return_intermediate:
            return torch.stack(states), torch.stack(refs)
        return out, ref_logits


@TRANSFORMER.register_module()
class Uni3DETRTransformer(nn.Module):
    def __init__(self, decoder=None, fp16_enabled=False, init_cfg=None, **kwargs):
        super().__init__()
        self.decoder = TRANSFORMER_LAYER_SEQUENCE.build(decoder)
        self.embed_dims = self.decoder.embed_dims
        self.d_model = 256
        if fp16_enabled:
            self.fp16_enabled = fp16_enabled

    def init_weights(self):
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        for m in self.modules():
            if isinstance(m, UniCrossAtten):
                m.init_weight()

    def forward(self, pts_value, query_embed, num_query, reg_branches=None, **kwargs):
        """pts_value [B,(1,)C,D,H,W]; query_embed [B, G*num_query, 256+3].  Returns the reference's triple:
        inter_states [L, G*nq, B, C], init_reference [B, G*nq, 3], inter_references [L, B, G*nq, 3] (sigmoid space)."""
        assert query_embed is not None
        if pts_value.dim() == 6:
            pts_value = pts_value.flatten(0, 1) if pts_value.shape[1] == 1 else pts_value[:, 0]
        parts = getattr(query_embed, "_u3d_parts", None)       # the head's fused query assembly leaves the two column blocks beside the cat
        init_sig = None
        if parts is not None and parts[0].shape[-1] == self.d_model:
            query, ref_logits, init_sig = parts                # (+ sigmoid(ref_logits): init_reference)
        else:
            ref_logits = query_embed[..., self.d_model:]
            query = query_embed[..., : self.d_model]
        states, refs = self.decoder.forward_bf(query, ref_logits, pts_value, reg_branches, num_query, ref_sig=init_sig)
        if not self.decoder.return_intermediate:
            states, refs = states[None], refs[None]
        refs_sig = getattr(self.decoder, "_refs_sig", None)     # written by the fused layer tails (plugin/fused_decoder._RefineDecode)
        if refs_sig is None or refs_sig.shape != refs.shape:
            refs_sig = refs.sigmoid()
        return states.permute(0, 2, 1, 3), (ref_logits.sigmoid() if init_sig is None else init_sig), refs_sig
