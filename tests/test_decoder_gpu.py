"""Fused decoder layer (u3d_decoder_layer_fwd/_bwd, u3d_mha_fwd/_bwd) against a plain-torch f32 restatement of the same layer
(ref: projects/mmdet3d_plugin/models/utils/uni3detr_transformer.py:145-212, 271-360; dense_heads/uni3detr_head.py:367-387).

The restatement runs in f32 on the bf16-rounded weights and rounds every tensor the kernels keep in bf16 (linear outputs,
activations): what is compared is the arithmetic, not the storage format.  Tolerances (stated, bf16 storage): 1.5e-2 relative L2 on
every forward tensor, 4e-2 on gradients.  Dropout is checked exactly: the kernels' keep masks are read back (u3d_dropout_mask) and
applied in the restatement.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import projects.mmdet3d_plugin  # noqa: F401
from uni3detr_amd import native as nv
from uni3detr_amd.configs.sunrgbd import model as MODEL_CFG
from uni3detr_amd.registry import build_model

pytestmark = pytest.mark.gpu


EXACT = [False]        # True: the restatement keeps f32 everywhere (the kernels' U3D_F32 instantiation), else it rounds through bf16


def R(t):
    return t if EXACT[0] else t.to(torch.bfloat16).float()


def rel(a, b):
    a, b = a.detach().float().reshape(-1), b.detach().float().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-12))


# ---------------------------------------------------------------------------------------------------------------------------
def attn_ref(qk, v, nq, keep=None, p=0.0):
    m = qk.shape[0]
    g = m // nq
    q = qk[:, :256].reshape(g, nq, 8, 32).transpose(1, 2)
    k = qk[:, 256:].reshape(g, nq, 8, 32).transpose(1, 2)
    vv = v.reshape(g, nq, 8, 32).transpose(1, 2)
    P = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(32.0), dim=-1)
    if keep is not None:
        P = P * keep.reshape(g, 8, nq, nq).float() / (1.0 - p)
    return (P @ vv).transpose(1, 2).reshape(m, 256)


@pytest.mark.parametrize("nq,groups", [(300, 6), (77, 3), (900, 2)])
def test_mha_forward_backward_match_torch(cuda, nq, groups):
    torch.manual_seed(nq)
    m = nq * groups
    qk = (torch.randn(m, 512, device=cuda) * 1.5).to(torch.bfloat16)
    v = torch.randn(m, 256, device=cuda).to(torch.bfloat16)
    o, lse = nv.mha_fwd(qk, v, nq)
    qf, vf = qk.float().requires_grad_(True), v.float().requires_grad_(True)
    ref = attn_ref(qf, vf, nq)
    assert rel(o, ref) < 1e-2, rel(o, ref)
    d_o = torch.randn(m, 256, device=cuda).to(torch.bfloat16)
    ref.backward(d_o.float())
    dqk, dv = nv.mha_bwd(qk, v, o, d_o, lse, nq)
    assert rel(dqk, qf.grad) < 2e-2, rel(dqk, qf.grad)
    assert rel(dv, vf.grad) < 2e-2, rel(dv, vf.grad)


def test_mha_dropout_uses_the_published_mask(cuda):
    torch.manual_seed(5)
    nq, groups, p, layer = 300, 3, 0.1, 2
    m = nq * groups
    rng = torch.tensor([0x1234567], dtype=torch.int64, device=cuda)
    qk = torch.randn(m, 512, device=cuda).to(torch.bfloat16)
    v = torch.randn(m, 256, device=cuda).to(torch.bfloat16)
    keep = nv.dropout_mask(rng, layer, 4, groups * 8 * nq * nq, p, cols=nq)
    rate = float(keep.float().mean())
    assert abs(rate - 0.9) < 5e-3, rate
    o, lse = nv.mha_fwd(qk, v, nq, p, layer, rng)
    qf, vf = qk.float().requires_grad_(True), v.float().requires_grad_(True)
    ref = attn_ref(qf, vf, nq, keep, p)
    assert rel(o, ref) < 1e-2, rel(o, ref)
    d_o = torch.randn(m, 256, device=cuda).to(torch.bfloat16)
    ref.backward(d_o.float())
    dqk, dv = nv.mha_bwd(qk, v, o, d_o, lse, nq, p, layer, rng)
    assert rel(dqk, qf.grad) < 2e-2 and rel(dv, vf.grad) < 2e-2, (rel(dqk, qf.grad), rel(dv, vf.grad))
    # another seed -> another mask
    rng2 = rng + 0x9E3779B1
    assert float((nv.dropout_mask(rng2, layer, 4, 100000, p, cols=nq)[:90000] != keep[:90000]).float().mean()) > 0.1


# ---------------------------------------------------------------------------------------------------------------------------
def ln(x, mod, relu=False):
    y = F.layer_norm(x, (256,), mod.weight, mod.bias, mod.eps)
    return y.relu() if relu else y


def lin(x, w, b):
    return x @ R(w).t() + b


def sine(ref):
    d = torch.arange(128, dtype=torch.float32, device=ref.device)
    dim_t = 10000 ** (2 * torch.div(d, 2, rounding_mode="floor") / 128)
    s = ref.sigmoid().unsqueeze(-1) * (2 * math.pi) / dim_t
    return torch.stack((s[..., 0::2].sin(), s[..., 1::2].cos()), dim=-1).flatten(-2).flatten(-2)


def restate(sp, lid, x, ref, rows_f, dims, masks=None, p=(0.0, 0.0), kact=None):
    """f32 restatement of one fused layer; returns a dict of the tensors the kernels save / emit.
    kact: {slot name: the kernels' own saved activation}: ReLU decisions are taken from it, so that a pre-activation that lands on
    the other side of zero by rounding noise (an O(1) difference in the gradient of that element) does not mask arithmetic errors."""
    B, qps, nq, D, H, W = dims
    L = sp.lin
    t = {}
    mk = (lambda i, v: v * masks[i].float() / (1 - p[1])) if masks is not None else (lambda i, v: v)

    class _Relu:
        def __init__(self, v):
            self.v = v

        def relu(self):
            return self.v.relu()

    def act(name, pre):
        """relu(pre), with the on/off decision of the kernels when their activation `name` is known"""
        if kact is None or name not in kact:
            return pre.relu()
        return pre * (kact[name].float() > 0).to(pre.dtype)
    t["SINE"] = R(sine(ref))
    t["RPH1"] = R(act("RPH1", lin(t["SINE"], L[nv.DL_RPH0][0], L[nv.DL_RPH0][3])))
    t["RPH2"] = R(act("RPH2", lin(t["RPH1"], L[nv.DL_RPH1][0], L[nv.DL_RPH1][3])))
    raw = R(lin(t["RPH2"], L[nv.DL_RPH2][0], L[nv.DL_RPH2][3]))
    xc = R(x)
    if lid > 0:
        t["QS1"] = R(act("QS1", lin(xc, L[nv.DL_QS0][0], L[nv.DL_QS0][3])))
        t["QS2"] = R(act("QS2", lin(t["QS1"], L[nv.DL_QS1][0], L[nv.DL_QS1][3])))
        t["QS"] = R(lin(t["QS2"], L[nv.DL_QS2][0], L[nv.DL_QS2][3]))
        t["RAW"] = raw
        t["POS"] = R(t["QS"] * raw)
    else:
        t["POS"] = raw
    t["QKIN"] = R(xc + t["POS"])
    ipw, ipb = L[nv.DL_INQK][0], L[nv.DL_INQK][3]
    t["QK"] = R(lin(t["QKIN"], ipw[:512], ipb[:512]))
    t["V"] = R(lin(xc, ipw[512:], ipb[512:]))
    t["O"] = R(attn_ref(t["QK"], t["V"], nq, None if masks is None else masks[4], p[0]))
    o2 = mk(0, R(lin(t["O"], L[nv.DL_OUTP][0], L[nv.DL_OUTP][3])))
    t["U1"] = x + o2
    x1 = ln(t["U1"], sp.ln[0])
    t["QP"] = R(R(x1) + t["POS"])
    wl = R(t["QP"] @ R(sp.attw.weight).t() + sp.attw.bias)
    t["WL"] = wl
    gate = R(wl.sigmoid())
    vol = rows_f.view(B, D, H, W, 256).permute(0, 4, 1, 2, 3)
    grid = ((ref.sigmoid() - 0.5) * 2).view(B, 1, 1, qps, 3)
    samp = F.grid_sample(vol, grid, align_corners=False).view(B, 256, qps).permute(0, 2, 1).reshape(-1, 256)
    t["SAMP"] = R(samp)
    t["GATED"] = R(t["SAMP"] * gate)
    out = mk(1, R(lin(t["GATED"], L[nv.DL_OPROJ][0], L[nv.DL_OPROJ][3])))
    p0 = R(R(ref) @ R(sp.pe0.weight).t() + sp.pe0.bias)
    t["P0"] = p0
    t["PEH0"] = R(act("PEH0", ln(p0, sp.ln[3])))
    t["UPE1"] = R(lin(t["PEH0"], L[nv.DL_PE1][0], L[nv.DL_PE1][3]))
    posfeat = R(act("POSFEAT", ln(t["UPE1"], sp.ln[4])))
    t["U2"] = x1 + out + posfeat
    x2 = ln(t["U2"], sp.ln[1])
    t["X2C"] = R(x2)
    if kact is not None and "FFH" in kact:      # saved after dropout: > 0 <=> kept and positive
        t["FFH"] = R(lin(t["X2C"], L[nv.DL_FFN0][0], L[nv.DL_FFN0][3])) * (kact["FFH"].float() > 0).float() / (1 - (p[1] if masks is not None else 0.0))
    else:
        t["FFH"] = mk(2, R(lin(t["X2C"], L[nv.DL_FFN0][0], L[nv.DL_FFN0][3]).relu()))
    f = mk(3, R(lin(t["FFH"], L[nv.DL_FFN1][0], L[nv.DL_FFN1][3])))
    t["U3"] = x2 + f
    x3 = ln(t["U3"], sp.ln[2])
    t["x_out"] = x3
    x3c = R(x3)
    t["R1"] = R(act("R1", lin(x3c, L[nv.DL_REG0][0], L[nv.DL_REG0][3])))
    t["R2"] = R(act("R2", lin(t["R1"], L[nv.DL_REG1][0], L[nv.DL_REG1][3])))
    t["reg"] = R(lin(t["R2"], L[nv.DL_REG2][0], L[nv.DL_REG2][3]))
    t["I1"] = R(act("I1", lin(x3c, L[nv.DL_IOU0][0], L[nv.DL_IOU0][3])))
    t["I2"] = R(act("I2", lin(t["I1"], L[nv.DL_IOU1][0], L[nv.DL_IOU1][3])))
    t["iou"] = R(lin(t["I2"], L[nv.DL_IOU2][0], L[nv.DL_IOU2][3])).squeeze(-1)
    t["UC1"] = R(lin(x3c, L[nv.DL_CLS0][0], L[nv.DL_CLS0][3]))
    t["C1"] = R(act("C1", ln(t["UC1"], sp.ln[5])))
    t["UC2"] = R(lin(t["C1"], L[nv.DL_CLS1][0], L[nv.DL_CLS1][3]))
    t["C2"] = R(act("C2", ln(t["UC2"], sp.ln[6])))
    t["cls"] = R(lin(t["C2"], L[nv.DL_CLS2][0], L[nv.DL_CLS2][3]))
    return t


SLOT_COLS = {"SINE": 384, "QK": 512, "FFH": 512}
GRAD_WS = []          # gradient workspaces of the fused backward calls (test hook: fused_decoder.DEBUG_KEEP)
F32_SLOTS = {"U1", "U2", "U3"}


def make_head(cuda, seed, train=True):
    torch.manual_seed(seed)
    head = build_model(MODEL_CFG).pts_bbox_head.to(cuda)
    with torch.no_grad():
        for m in head.modules():                       # non-trivial gate and norm parameters
            if hasattr(m, "attention_weights"):
                m.attention_weights.weight.normal_(0, 0.05)
                m.attention_weights.bias.normal_(0, 0.5)
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
    return head.train(train)


def run_layer(cuda, lid, p_on, seed=0, et=torch.bfloat16):
    from uni3detr_amd.plugin import fused_decoder as fdm
    head = make_head(cuda, seed)
    dec = head.transformer.decoder
    fd = fdm.FusedDecoder(dec, head.reg_branches, head.cls_branches, head.iou_branches)
    sp = fd.specs[lid]
    if not p_on:
        sp.p_attn = sp.p_drop = 0.0
    B, G, nq, D, H, W = 2, 3, 300, 15, 40, 40
    M = B * G * nq
    g = torch.Generator(device="cpu").manual_seed(seed + 17)
    x = (torch.randn(M, 256, generator=g) * 0.7).to(cuda).requires_grad_(True)
    ref = (torch.randn(M, 3, generator=g) * 1.2).to(cuda).requires_grad_(lid == 0)
    rows_f = torch.randn(B * D * H * W, 256, generator=g).to(cuda).to(torch.bfloat16).float().requires_grad_(True)
    fd.refresh(cuda, et)
    fd.rng.fill_(0x2545F4914F6C + seed)
    dims = (B, G * nq, nq, D, H, W)
    rows = rows_f.to(et)
    meta = (fd, lid, dims, None, et)
    outs = fdm.FusedLayerFn.apply(x, None, ref, rows, meta, *fdm.tensor_list(sp))
    return head, fd, sp, (x, ref, rows_f), dims, outs


@pytest.mark.parametrize("lid", [0, 1])
def test_fused_layer_forward_matches_restatement(cuda, lid):
    head, fd, sp, (x, ref, rows_f), dims, outs = run_layer(cuda, lid, p_on=False)
    x_out, xc_out, reg, cls, iou = outs
    with torch.no_grad():
        t = restate(sp, lid, x, ref, rows_f, dims)
    M = x.shape[0]
    so, _ = nv.decoder_layer_slots(M, sp.ncls, sp.code)
    # the save buffer is the last saved tensor of the autograd node
    save = x_out.grad_fn.saved_tensors[5]
    bad = []
    for name in nv.DS_NAMES:
        if name not in t or name in ("WL",):
            continue
        cols = SLOT_COLS.get(name, 256)
        got = nv.slot_view(save, so[name], M, cols, torch.float32 if name in F32_SLOTS else torch.bfloat16)
        e = rel(got, t[name])
        if e > 1.5e-2:
            bad.append((name, e))
    wl = nv.slot_view(save, so["MR"], M, 16, torch.float32)[:, 14]
    if rel(wl, t["WL"].squeeze(-1)) > 1.5e-2:
        bad.append(("WL", rel(wl, t["WL"].squeeze(-1))))
    for name, got in (("x_out", x_out), ("reg", reg), ("cls", cls), ("iou", iou)):
        e = rel(got, t[name])
        if e > 1.5e-2:
            bad.append((name, e))
    assert rel(xc_out, x_out) < 4e-3
    assert not bad, bad


def _grad_compare(cuda, lid, p_on):
    head, fd, sp, (x, ref, rows_f), dims, outs = run_layer(cuda, lid, p_on=p_on, seed=3)
    x_out, xc_out, reg, cls, iou = outs
    M = x.shape[0]
    g = torch.Generator(device="cpu").manual_seed(99)
    cots = [torch.randn(o.shape, generator=g).to(cuda) for o in (x_out, reg, cls, iou)]
    from uni3detr_amd.plugin import fused_decoder as fdm
    plist = list(dict.fromkeys(fdm.tensor_list(sp)))
    loss = sum((o * c).sum() for o, c in zip((x_out, reg, cls, iou), cots))
    inputs = [x, rows_f] + ([ref] if lid == 0 else []) + plist
    save = x_out.grad_fn.saved_tensors[5]
    fdm.DEBUG_KEEP = GRAD_WS
    got = torch.autograd.grad(loss, inputs, allow_unused=True)
    fdm.DEBUG_KEEP = None
    masks = None
    p = (sp.p_attn, sp.p_drop)
    if p_on:
        G8 = (M // dims[2]) * 8
        masks = {0: nv.dropout_mask(fd.rng, lid, 0, M * 256, p[1]).view(M, 256), 1: nv.dropout_mask(fd.rng, lid, 1, M * 256, p[1]).view(M, 256),
                 2: nv.dropout_mask(fd.rng, lid, 2, M * 512, p[1]).view(M, 512), 3: nv.dropout_mask(fd.rng, lid, 3, M * 256, p[1]).view(M, 256),
                 4: nv.dropout_mask(fd.rng, lid, 4, G8 * dims[2] * dims[2], p[0], cols=dims[2])}
    so, go = nv.decoder_layer_slots(M, sp.ncls, sp.code)
    kact = {n: nv.slot_view(save, so[n], M, SLOT_COLS.get(n, 256), torch.bfloat16) for n in ("RPH1", "RPH2", "QS1", "QS2", "R1", "R2", "I1", "I2", "FFH", "PEH0", "C1", "C2")}
    upe1 = nv.slot_view(save, so["UPE1"], M, 256, torch.bfloat16).float()
    kact["POSFEAT"] = ln(upe1, sp.ln[4])
    t = restate(sp, lid, x, ref, rows_f, dims, masks, p, kact)
    for name, o in (("x_out", x_out), ("reg", reg), ("cls", cls), ("iou", iou)):
        assert rel(o, t[name]) < 1.5e-2, (name, rel(o, t[name]))
    loss_r = sum((t[n] * c).sum() for n, c in zip(("x_out", "reg", "cls", "iou"), cots))
    inter = ["U1", "O", "QK", "V", "UPE1", "UC1", "UC2", "P0", "POS", "U2", "U3"]
    res = torch.autograd.grad(loss_r, inputs + [t[n] for n in inter], allow_unused=True)
    want, igrads = res[:len(inputs)], dict(zip(inter, res[len(inputs):]))
    if os.environ.get("U3D_TEST_DUMP") and GRAD_WS:
        gws = GRAD_WS[-1]
        with open(os.environ["U3D_TEST_DUMP"], "a") as fh:
            fh.write(f"--- slots lid {lid}\n")
            for sname, tname, cols, dt in (("DU1", "U1", 256, torch.float32), ("DO", "O", 256, torch.bfloat16), ("DQK", "QK", 512, torch.bfloat16),
                                           ("DV", "V", 256, torch.bfloat16), ("UPE1", "UPE1", 256, torch.bfloat16), ("C1U", "UC1", 256, torch.bfloat16),
                                           ("C2U", "UC2", 256, torch.bfloat16), ("P0", "P0", 256, torch.bfloat16)):
                fh.write(f"{rel(nv.slot_view(gws, go[sname], M, cols, dt), igrads[tname]):.4f} {float(igrads[tname].norm()):.3e} slot {sname}\n")
    names = ["x", "rows"] + (["ref"] if lid == 0 else [])
    pnames = {id(p_): n for n, p_ in head.named_parameters()}
    names += [pnames.get(id(p_), "?") for p_ in plist]
    bad = []
    for n, a, b in zip(names, got, want):
        if b is None or float(b.abs().max()) == 0.0:
            assert a is None or float(a.abs().max()) < 1e-6 or lid == 0, n       # unused (query_scale in layer 0)
            continue
        assert a is not None, n
        e = rel(a, b)
        if e > 4e-2:
            bad.append((n, e, float(b.norm())))
    if os.environ.get("U3D_TEST_DUMP"):
        with open(os.environ["U3D_TEST_DUMP"], "a") as fh:
            fh.write(f"--- lid {lid} dropout {p_on}\n")
            for n, a, b in zip(names, got, want):
                if b is not None and a is not None and float(b.abs().max()) > 0:
                    fh.write(f"{rel(a, b):.4f} {float(b.norm()):.3e} {n}\n")
    assert not bad, bad


@pytest.mark.parametrize("lid", [0, 2])
def test_fused_layer_gradients_match_restatement(cuda, lid):
    _grad_compare(cuda, lid, p_on=False)


def test_fused_layer_with_dropout_matches_restatement_with_the_same_masks(cuda):
    _grad_compare(cuda, 1, p_on=True)


def test_head_bf16_fused_path_matches_layerwise_path(cuda):
    """Whole head in bf16 mode: fused decoder vs the layer-by-layer (torch op) formulation of the same modules."""
    from uni3detr_amd.plugin import fused_decoder as fdm
    head = make_head(cuda, 11)
    for m in head.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if hasattr(m, "attn_drop"):
            m.attn_drop = 0.0
    g = torch.Generator(device="cpu").manual_seed(5)
    feats = torch.randn(2, 256, 15, 40, 40, generator=g).clamp_min(0).to(cuda).to(memory_format=torch.channels_last_3d)
    fps = torch.rand(2, 600, 3, generator=g).to(cuda)
    res = {}
    for fused in (True, False):
        fdm.ENABLED = fused
        f = feats.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            outs = head(f, None, fps)
        tot = sum((v.float() ** 2).sum() * w for v, w in zip((outs["all_cls_scores"], outs["all_bbox_preds"], outs["all_iou_preds"]), (1.0, 0.1, 1.0)))
        head.zero_grad(set_to_none=True)
        tot.backward()
        res[fused] = ({k: v.detach().float() for k, v in outs.items()}, f.grad.float(),
                      {n: p.grad.detach().clone() for n, p in head.named_parameters() if p.grad is not None})
    fdm.ENABLED = True
    for k in res[True][0]:
        assert rel(res[True][0][k], res[False][0][k]) < 3e-2, (k, rel(res[True][0][k], res[False][0][k]))
    # the volume gradient passes through every ReLU / LayerNorm+ReLU decision of both formulations: an activation that lands on the other
    # side of zero by rounding noise changes that element's gradient by O(1), so two bf16 formulations agree less tightly here than
    # the fused kernels agree with their own restatement (4e-2 with the kernels' decisions, tests above)
    assert rel(res[True][1], res[False][1]) < 1.2e-1
    bad = [(n, rel(gv, res[False][2][n])) for n, gv in res[True][2].items() if n in res[False][2] and rel(gv, res[False][2][n]) > 8e-2
           and float(res[False][2][n].norm()) > 1e-6]
    assert not bad, bad
    assert set(res[True][2]) == set(res[False][2])


@pytest.mark.parametrize("spread", [1.0, 0.02], ids=["spread", "clustered"])
def test_packed_bf16_volume_gradient_scatter_vs_f32_accumulator(cuda, spread):
    """the OPT-IN bf16 accumulator (fused_decoder.PK_SCATTER) collects the value-volume gradient of all 3 layers in ONE bf16
    buffer; each layer's per-cell sum (f32, fixed order: native.value_scatter) is rounded to 8 mantissa bits as it is added.  Measured
    against the f32 accumulator (the default) with the queries spread over the volume and with all 600 FPS queries of a scene inside a
    2 % cube.  Gates: spread <= 1 %, clustered <= 15 %."""
    from uni3detr_amd.plugin import fused_decoder as fdm
    head = make_head(cuda, 11)
    for m in head.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if hasattr(m, "attn_drop"):
            m.attn_drop = 0.0
    g = torch.Generator(device="cpu").manual_seed(5)
    feats = torch.randn(2, 256, 15, 40, 40, generator=g).clamp_min(0).to(cuda).to(memory_format=torch.channels_last_3d)
    fps = (0.5 + (torch.rand(2, 600, 3, generator=g) - 0.5) * spread).to(cuda)
    res = {}
    old = fdm.PK_SCATTER
    try:
        for pk in (True, False):
            fdm.PK_SCATTER = pk
            f = feats.clone().requires_grad_(True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                outs = head(f, None, fps)
            tot = sum((v.float() ** 2).sum() * w for v, w in zip((outs["all_cls_scores"], outs["all_bbox_preds"], outs["all_iou_preds"]), (1.0, 0.1, 1.0)))
            head.zero_grad(set_to_none=True)
            tot.backward()
            res[pk] = f.grad.float()
    finally:
        fdm.PK_SCATTER = old
    e = rel(res[True], res[False])
    nz = int((res[False].abs().sum(1) > 0).sum())
    print(f"\n[pk scatter] spread {spread}: rel L2 {e:.4f} vs f32 accumulator, {nz} touched cells")
    assert e <= (1e-2 if spread == 1.0 else 0.15), e


@pytest.mark.parametrize("lid", [0, 2])
def test_fused_layer_backward_is_deterministic(cuda, lid):
    """Every gradient slot of the fused backward is bitwise reproducible (NaN-poisoned workspaces: a read-before-write would show).
    Guards against the exec-mask miscompilation described in csrc/decoder_common.h, which surfaced as run-to-run differences in
    single rows of each 32-row block."""
    from uni3detr_amd.plugin import fused_decoder as fdm
    first = None
    fdm.POISON = True
    try:
        for it in range(6):
            head, fd, sp, (x, ref, rows_f), dims, outs = run_layer(cuda, lid, p_on=True, seed=3)
            x_out, xc_out, reg, cls, iou = outs
            M = x.shape[0]
            g = torch.Generator(device="cpu").manual_seed(99)
            cots = [torch.randn(o.shape, generator=g).to(cuda) for o in (x_out, reg, cls, iou)]
            loss = sum((o * c).sum() for o, c in zip((x_out, reg, cls, iou), cots))
            ws = []
            fdm.DEBUG_KEEP = ws
            dx, = torch.autograd.grad(loss, [x])
            fdm.DEBUG_KEEP = None
            _, go = nv.decoder_layer_slots(M, sp.ncls, sp.code)
            snap = {n: nv.slot_view(ws[-1], go[n], M, {"FFH": 512, "DQK": 512}.get(n, 256), torch.float32 if n == "DU1" else torch.bfloat16).clone()
                    for n in ("C2U", "C1U", "I1", "R1", "F", "FFH", "UPE1", "P0", "OUT", "DU1", "DO", "DQK", "DV", "RAW", "RPH2", "RPH1") + (("QS", "QS1") if lid else ())}
            snap["dx"] = dx.clone()
            snap["lnp"] = nv.slot_view(ws[-1], go["LNP"], nv.DL_NLN * 2 * fdm.d_blocks(M), 256, torch.float32).clone()
            assert all(bool(torch.isfinite(v.float()).all()) for v in snap.values())
            if first is None:
                first = snap
            else:
                for k, v in snap.items():
                    assert torch.equal(v, first[k]), (it, k)
    finally:
        fdm.POISON = False
        fdm.DEBUG_KEEP = None


def _two_layer_param_grads(cuda, head, fd, et, scope, shared_defer):
    """Layers 0 and 1 chained as fused_decoder.run chains them (ref_point_head is used by both, query_scale by layer 1 only), M = 40
    rows, one backward; -> {parameter name: gradient} over both layers' tensor_list."""
    import contextlib
    from uni3detr_amd.plugin import fused_decoder as fdm
    from uni3detr_amd.plugin import transformer as T
    B, nq, D, H, W = 1, 40, 3, 4, 5                  # the shapes of tests/test_decoder_waves_gpu.py
    g = torch.Generator(device="cpu").manual_seed(23)
    x = (torch.randn(B * nq, 256, generator=g) * 0.7).to(cuda).requires_grad_(True)
    ref = (torch.randn(B * nq, 3, generator=g) * 1.2).to(cuda)
    rows = torch.randn(B * D * H * W, 256, generator=g).to(cuda).to(et)
    fd.refresh(cuda, et)
    fd.rng.fill_(0x2545F4914F6C)
    T.reset_param_uses()
    outs, xc = [], None
    for lid in (0, 1):
        x, xc, reg, cls, iou = fdm.FusedLayerFn.apply(x, xc, ref, rows, (fd, lid, (B, nq, nq, D, H, W), None, et), *fdm.tensor_list(fd.specs[lid]))
        ref = ref + reg.detach()[:, [0, 1, 4]]
        outs += [x, reg, cls, iou]
    loss = sum((o * torch.randn(o.shape, generator=g).to(cuda)).sum() for o in outs)
    head.zero_grad(set_to_none=True)
    old = fdm.SHARED_DEFER
    fdm.SHARED_DEFER = shared_defer
    try:
        with (T.deferred_param_grads() if scope else contextlib.nullcontext()):
            loss.backward()
    finally:
        fdm.SHARED_DEFER = old
    names = {id(p): n for n, p in head.named_parameters()}
    params = dict.fromkeys(t for lid in (0, 1) for t in fdm.tensor_list(fd.specs[lid]))
    return {names[id(p)]: p.grad.clone() for p in params}


@pytest.mark.parametrize("mode", ["bf16", "f32", "f32_split"])
def test_parameter_gradients_do_not_depend_on_the_route(cuda, mode):
    """Every parameter gradient of two chained fused layers computed (a) outside a deferred scope, (b) inside one, (c) inside one with
    SHARED_DEFER off, under POISON (a placeholder nobody writes is NaN).  M = 40: one full 32-row block plus a partial one, so the
    LayerNorm block partials and a linear shared by two layers (ref_point_head) both occur.
    Measured before the route moved into plugin/param_grads.py: f32 and f32_split - all 108 gradients torch.equal in (a), (b), (c);
    bf16 - (c) torch.equal to (a), (b) torch.equal but for ref_point_head.layers.2.bias at relative L2 1.3424e-08 (the batched launch
    adds the two uses' column sums in another order than autograd adds two finished sums).  That one is held to twice the figure
    (run-to-run slack of an order-dependent f32 sum), everything else to torch.equal."""
    from uni3detr_amd.plugin import fused_decoder as fdm
    et = torch.bfloat16 if mode == "bf16" else torch.float32
    head = make_head(cuda, 7)
    head.transformer.decoder.split_f32_wgrad = mode == "f32_split"
    fd = fdm.FusedDecoder(head.transformer.decoder, head.reg_branches, head.cls_branches, head.iou_branches)
    for sp in fd.specs:
        sp.p_attn = sp.p_drop = 0.0
    fdm.POISON = True
    try:
        a, b, c = (_two_layer_param_grads(cuda, head, fd, et, scope, shared) for scope, shared in ((False, True), (True, True), (True, False)))
    finally:
        fdm.POISON = False
    assert len(a) == 108 and set(a) == set(b) == set(c)
    bound = {("bf16", "b", "transformer.decoder.ref_point_head.layers.2.bias"): 2 * 1.3424e-08}
    differ = {}
    for tag, other in (("b", b), ("c", c)):
        for n, ga in a.items():
            assert bool(torch.isfinite(ga).all()) and bool(torch.isfinite(other[n]).all()), (mode, tag, n)
            if not torch.equal(ga, other[n]):
                differ[(mode, tag, n)] = rel(other[n], ga)
    print(f"\n[param grad routes] {mode}: differing from (a): {differ}")
    assert all(e <= bound.get(key, 0.0) for key, e in differ.items()), differ


# ---------------------------------------------------------------------------------------------------------------------------
# U3D_F32 instantiation of the SAME kernels (csrc/decoder_common.h: element trait EF, exact v_mfma_f32_16x16x4_f32): the parity-grade
# decoder.  Tolerances: 2e-5 relative L2 forward and on gradients (measured ~1e-6) - f32 arithmetic against torch's f32 ops, no storage rounding.
# ReLU decisions are the restatement's own, except for elements PROVEN to be rounding ties (see the gradient test).
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,groups", [(300, 6), (77, 3), (900, 2)])
def test_mha_f32_forward_backward_match_torch(cuda, nq, groups):
    torch.manual_seed(nq)
    m = nq * groups
    qk = torch.randn(m, 512, device=cuda) * 1.5
    v = torch.randn(m, 256, device=cuda)
    o, lse = nv.mha_fwd(qk, v, nq)
    assert o.dtype == torch.float32
    qf, vf = qk.clone().requires_grad_(True), v.clone().requires_grad_(True)
    ref = attn_ref(qf, vf, nq)
    assert rel(o, ref) < 2e-5, rel(o, ref)
    d_o = torch.randn(m, 256, device=cuda)
    ref.backward(d_o)
    dqk, dv = nv.mha_bwd(qk, v, o, d_o, lse, nq)
    assert rel(dqk, qf.grad) < 1e-4, rel(dqk, qf.grad)
    assert rel(dv, vf.grad) < 1e-4, rel(dv, vf.grad)


def test_mha_f32_dropout_uses_the_same_mask_as_bf16(cuda):
    torch.manual_seed(6)
    nq, groups, p, layer = 300, 2, 0.1, 1
    m = nq * groups
    rng = torch.tensor([0x7654321], dtype=torch.int64, device=cuda)
    qk, v = torch.randn(m, 512, device=cuda), torch.randn(m, 256, device=cuda)
    keep = nv.dropout_mask(rng, layer, 4, groups * 8 * nq * nq, p, cols=nq)
    o, lse = nv.mha_fwd(qk, v, nq, p, layer, rng)
    qf, vf = qk.clone().requires_grad_(True), v.clone().requires_grad_(True)
    ref = attn_ref(qf, vf, nq, keep, p)
    assert rel(o, ref) < 2e-5, rel(o, ref)
    d_o = torch.randn(m, 256, device=cuda)
    ref.backward(d_o)
    dqk, dv = nv.mha_bwd(qk, v, o, d_o, lse, nq, p, layer, rng)
    assert rel(dqk, qf.grad) < 1e-4 and rel(dv, vf.grad) < 1e-4, (rel(dqk, qf.grad), rel(dv, vf.grad))


@pytest.fixture
def exact():
    EXACT[0] = True
    yield
    EXACT[0] = False


@pytest.mark.parametrize("lid", [0, 1])
def test_fused_layer_f32_forward_matches_f32_restatement(cuda, exact, lid):
    f32 = torch.float32
    head, fd, sp, (x, ref, rows_f), dims, outs = run_layer(cuda, lid, p_on=False, et=f32)
    x_out, xc_out, reg, cls, iou = outs
    with torch.no_grad():
        t = restate(sp, lid, x, ref, rows_f, dims)
    M = x.shape[0]
    so, _ = nv.decoder_layer_slots(M, sp.ncls, sp.code, f32)
    save = x_out.grad_fn.saved_tensors[5]
    bad = []
    for name in nv.DS_NAMES:
        if name not in t or name in ("WL",):
            continue
        got = nv.slot_view(save, so[name], M, SLOT_COLS.get(name, 256), f32)
        e = rel(got, t[name])
        if e > 2e-5:
            bad.append((name, e))
    wl = nv.slot_view(save, so["MR"], M, 16, f32)[:, 14]
    if rel(wl, t["WL"].squeeze(-1)) > 2e-5:
        bad.append(("WL", rel(wl, t["WL"].squeeze(-1))))
    for name, got in (("x_out", x_out), ("reg", reg), ("cls", cls), ("iou", iou)):
        e = rel(got, t[name])
        if e > 2e-5:
            bad.append((name, e))
    assert not bad, bad


@pytest.mark.parametrize("lid,p_on", [(0, False), (2, False), (1, True)])
def test_fused_layer_f32_gradients_match_f32_restatement(cuda, exact, lid, p_on):
    from uni3detr_amd.plugin import fused_decoder as fdm
    f32 = torch.float32
    head, fd, sp, (x, ref, rows_f), dims, outs = run_layer(cuda, lid, p_on=p_on, seed=3, et=f32)
    x_out, xc_out, reg, cls, iou = outs
    M = x.shape[0]
    g = torch.Generator(device="cpu").manual_seed(99)
    cots = [torch.randn(o.shape, generator=g).to(cuda) for o in (x_out, reg, cls, iou)]
    plist = list(dict.fromkeys(fdm.tensor_list(sp)))
    loss = sum((o * c).sum() for o, c in zip((x_out, reg, cls, iou), cots))
    inputs = [x, rows_f] + ([ref] if lid == 0 else []) + plist
    save = x_out.grad_fn.saved_tensors[5]
    got = torch.autograd.grad(loss, inputs, allow_unused=True)
    masks, p = None, (sp.p_attn, sp.p_drop)
    if p_on:
        G8 = (M // dims[2]) * 8
        masks = {0: nv.dropout_mask(fd.rng, lid, 0, M * 256, p[1]).view(M, 256), 1: nv.dropout_mask(fd.rng, lid, 1, M * 256, p[1]).view(M, 256),
                 2: nv.dropout_mask(fd.rng, lid, 2, M * 512, p[1]).view(M, 512), 3: nv.dropout_mask(fd.rng, lid, 3, M * 256, p[1]).view(M, 256),
                 4: nv.dropout_mask(fd.rng, lid, 4, G8 * dims[2] * dims[2], p[0], cols=dims[2])}
    with torch.no_grad():
        t = restate(sp, lid, x, ref, rows_f, dims, masks, p)          # the restatement's OWN ReLU decisions
    for name, o in (("x_out", x_out), ("reg", reg), ("cls", cls), ("iou", iou)):
        assert rel(o, t[name]) < 2e-5, (name, rel(o, t[name]))
    # ReLU ties: two f32 formulations sum in different orders, so of the ~6 M activations of a layer a handful have pre-activations
    # within rounding of zero and land on different sides - an O(1) change of that element's gradient (2e-3 of a bias gradient for
    # ONE element).  Such elements are COUNTED and PROVEN to be ties (both activations < 1e-5 in magnitude); the gradient comparison
    # then uses the kernels' decision for them.  Everything else is the restatement's own arithmetic.
    so, _ = nv.decoder_layer_slots(M, sp.ncls, sp.code, f32)
    relu_slots = ("RPH1", "RPH2", "R1", "R2", "I1", "I2", "FFH", "PEH0", "C1", "C2") + (("QS1", "QS2") if lid else ())
    kact = {n: nv.slot_view(save, so[n], M, SLOT_COLS.get(n, 256), f32) for n in relu_slots}
    kact["POSFEAT"] = ln(nv.slot_view(save, so["UPE1"], M, 256, f32), sp.ln[4]).detach()
    flips = 0
    for n in relu_slots:
        diff = (kact[n] > 0) != (t[n] > 0)
        k = int(diff.sum())
        if k:
            assert float(torch.maximum(kact[n].abs(), t[n].abs())[diff].max()) < 1e-5, n      # a tie, not an arithmetic error
        flips += k
    assert flips <= 64, flips
    print(f"f32 fused layer {lid} dropout={p_on}: {flips} ReLU tie(s) among the saved activations")
    t = restate(sp, lid, x, ref, rows_f, dims, masks, p, kact)
    loss_r = sum((t[n] * c).sum() for n, c in zip(("x_out", "reg", "cls", "iou"), cots))
    want = torch.autograd.grad(loss_r, inputs, allow_unused=True)
    names = ["x", "rows"] + (["ref"] if lid == 0 else [])
    pnames = {id(p_): n for n, p_ in head.named_parameters()}
    names += [pnames.get(id(p_), "?") for p_ in plist]
    bad, worst = [], 0.0
    for n, a, b in zip(names, got, want):
        if b is None or float(b.abs().max()) == 0.0:
            continue
        assert a is not None, n
        e = rel(a, b)
        worst = max(worst, e)
        if e > 2e-5:
            bad.append((n, e, float(b.norm())))
    print(f"f32 fused layer {lid} dropout={p_on}: worst relative gradient error {worst:.2e}")
    assert not bad, bad


def test_uncovered_decoder_call_raises_instead_of_running_vendor_kernels(cuda):
    """there is no vendor-kernel (F.linear / SDPA) decoder a user can switch on.  A CUDA call in a layout the fused HIP
    decoder does not cover (here: float16 autocast) fails loudly; the layer-by-layer formulation is only reachable when a test flips
    fused_decoder.ENABLED in-process (the A/B comparisons above), and no environment variable selects it."""
    import os
    from uni3detr_amd.plugin import fused_decoder as fdm
    from uni3detr_amd.plugin import transformer as T
    assert fdm.ENABLED is True and not hasattr(T, "ALLOW_ATEN_DECODER")
    for name in ("U3D_ALLOW_ATEN_DECODER", "U3D_FUSED_DECODER", "U3D_UNSAFE_LINEAR"):
        src = open(T.__file__).read() + open(fdm.__file__).read()
        assert f'"{name}"' not in src and f"'{name}'" not in src, name
    head = make_head(cuda, 11)
    g = torch.Generator(device="cpu").manual_seed(5)
    feats = torch.randn(1, 256, 15, 40, 40, generator=g).clamp_min(0).to(cuda).to(memory_format=torch.channels_last_3d).requires_grad_(True)
    fps = torch.rand(1, 600, 3, generator=g).to(cuda)
    with pytest.raises(RuntimeError, match="no vendor-kernel"):
        with torch.autocast("cuda", dtype=torch.float16):
            head(feats, None, fps)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_value_scatter_sums_each_cell_in_a_fixed_order(cuda, dt):
    """native.value_scatter against a float64 index_add of the same records: out-of-volume corners (-1) skipped, cells with more
    entries than the kernel's id list (one cell takes 300) summed too, and the result bitwise the same on every call."""
    g = torch.Generator(device="cpu").manual_seed(17)
    m, cells = 2000, 5000
    ds = torch.randn(m, 256, generator=g)
    cell = torch.randint(0, cells, (m, 8), generator=g, dtype=torch.int32)
    cell[torch.rand(m, 8, generator=g) < 0.1] = -1
    cell[:300, 0] = 7                                           # a crowded cell: beyond the per-cell id list
    cell[300:310, :] = 11                                       # one row hitting the same cell with all eight corners
    w = torch.rand(m, 8, generator=g)
    rec = torch.cat([ds.reshape(-1).view(torch.uint8), cell.reshape(-1).view(torch.uint8), w.reshape(-1).view(torch.uint8)]).to(cuda)
    assert rec.numel() == nv.lib().u3d_value_records_bytes(m)
    ref = torch.zeros(cells, 256, dtype=torch.float64)
    ok = cell.reshape(-1) >= 0
    rows = torch.arange(m).repeat_interleave(8)[ok]
    ref.index_add_(0, cell.reshape(-1)[ok].long(), ds.double()[rows] * w.reshape(-1)[ok].double()[:, None])
    outs = []
    for _ in range(3):
        dv = torch.zeros(cells, 256, dtype=dt, device=cuda)
        nv.value_scatter(rec, m, dv)
        outs.append(dv)
    assert all(torch.equal(o, outs[0]) for o in outs[1:])
    got = outs[0].double().cpu()
    tol = 1e-5 if dt == torch.float32 else 8e-3                 # one f32 sum per cell; bf16: rounded once on the way in
    assert float((got - ref).abs().max()) <= tol * float(ref.abs().max())
    assert bool((got[ref.abs().sum(1) == 0] == 0).all())


@pytest.mark.parametrize("spread", [1.0, 0.02], ids=["spread", "clustered"])
def test_value_volume_gradient_is_bitwise_reproducible(cuda, spread):
    """The gradient w.r.t. the sampled feature volume - the one the neck, backbone and encoder backward start from - is the same bit for
    bit on every run of the same step (queries spread over the volume, and clustered so that cells collect hundreds of contributions)."""
    head = make_head(cuda, 11)
    for mod in head.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if hasattr(mod, "attn_drop"):
            mod.attn_drop = 0.0
    g = torch.Generator(device="cpu").manual_seed(5)
    feats = torch.randn(2, 256, 15, 40, 40, generator=g).clamp_min(0).to(cuda).to(memory_format=torch.channels_last_3d)
    fps = (0.5 + (torch.rand(2, 600, 3, generator=g) - 0.5) * spread).to(cuda)
    grads = []
    for _ in range(3):
        f = feats.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            outs = head(f, None, fps)
        tot = sum((v.float() ** 2).sum() * w for v, w in zip((outs["all_cls_scores"], outs["all_bbox_preds"], outs["all_iou_preds"]), (1.0, 0.1, 1.0)))
        head.zero_grad(set_to_none=True)
        tot.backward()
        grads.append(f.grad.clone())
    assert float(grads[0].abs().sum()) > 0
    assert all(torch.equal(x, grads[0]) for x in grads[1:])
