"""The bf16 row-chain kernels of the fused decoder layer (k_dec_pre / k_dec_post and their backward, csrc/decoder.hip, decoder_bwd.hip)
at eight waves per workgroup against the SAME kernels at four (element traits EB / EB4, fused_decoder.ROW_WAVES).  The wave count
only deals output columns and rows to waves: every output element is still produced by the same MFMAs in the same order, a row's
reductions stay inside one wave, and the LayerNorm (dgamma, dbeta) partials keep their row order (dc_layernorm_bwd) - so the two must
agree BIT FOR BIT: torch.equal, no tolerance.

Shapes are the smallest that can still go wrong (one scene, one query group, a 3 x 4 x 5 volume): M = 40 (a full 32-row block and one
with 8 live + 24 clamped rows), M = 32 (exactly one block), M = 1 (a single live row)."""
import pytest
import torch

import projects.mmdet3d_plugin  # noqa: F401
from uni3detr_amd import native as nv

from test_decoder_gpu import make_head

pytestmark = pytest.mark.gpu

D, H, W = 3, 4, 5
_HEAD = {}


def _fused(cuda):
    """One head + FusedDecoder for the whole module (the parameters are inputs here, never updated)."""
    from uni3detr_amd.plugin import fused_decoder as fdm
    if "fd" not in _HEAD:
        head = make_head(cuda, 5)
        fd = fdm.FusedDecoder(head.transformer.decoder, head.reg_branches, head.cls_branches, head.iou_branches)
        fd.refresh(cuda, torch.bfloat16)
        _HEAD["head"], _HEAD["fd"] = head, fd
        _HEAD["p"] = [(sp.p_attn, sp.p_drop) for sp in fd.specs]
    return _HEAD["fd"]


def _run(cuda, fd, lid, m, p_on, waves):
    """One fused layer forward + backward from seeded inputs at `waves` row waves: dict name -> tensor of everything it produced."""
    from uni3detr_amd.plugin import fused_decoder as fdm
    sp = fd.specs[lid]
    sp.p_attn, sp.p_drop = _HEAD["p"][lid] if p_on else (0.0, 0.0)
    g = torch.Generator(device="cpu").manual_seed(1000 + m)
    x = (torch.randn(m, 256, generator=g) * 0.7).to(cuda).requires_grad_(True)
    ref = (torch.randn(m, 3, generator=g) * 1.2).to(cuda).requires_grad_(lid == 0)
    rows = torch.randn(D * H * W, 256, generator=g).to(cuda).to(torch.bfloat16).requires_grad_(True)
    cots = [torch.randn(s, generator=g).to(cuda) for s in ((m, 256), (m, sp.code), (m, sp.ncls), (m,))]
    fd.rng.fill_(0x2545F4914F6C + lid)                       # the same rng words for both wave counts
    plist = list(dict.fromkeys(fdm.tensor_list(sp)))
    ws = []
    old = fdm.ROW_WAVES, fdm.POISON, fdm.DEBUG_KEEP
    fdm.ROW_WAVES, fdm.POISON, fdm.DEBUG_KEEP = waves, True, ws      # NaN-filled workspaces: bytes nobody writes compare equal too
    try:
        meta = (fd, lid, (1, m, m, D, H, W), None, torch.bfloat16)
        x_out, xc_out, reg, cls, iou = fdm.FusedLayerFn.apply(x, None, ref, rows, meta, *fdm.tensor_list(sp))
        save = x_out.grad_fn.saved_tensors[5]
        loss = sum((o * c).sum() for o, c in zip((x_out, reg, cls, iou), cots))
        grads = torch.autograd.grad(loss, [x, rows] + ([ref] if lid == 0 else []) + plist, allow_unused=True)
    finally:
        fdm.ROW_WAVES, fdm.POISON, fdm.DEBUG_KEEP = old
    out = {"x_out": x_out, "xc_out": xc_out, "reg": reg, "cls": cls, "iou": iou, "dx": grads[0], "drows": grads[1]}
    k = 2
    if lid == 0:
        out["dref"] = grads[2]
        k = 3
    pnames = {id(p_): n for n, p_ in _HEAD["head"].named_parameters()}
    for p_, gp in zip(plist, grads[k:]):
        if gp is not None:                                   # query_scale is unused in layer 0
            out["d " + pnames.get(id(p_), "?")] = gp
    out = {n: t.detach().clone() for n, t in out.items()}
    out["save slots"] = save.clone()
    out["gradient workspace"] = ws[-1].clone()
    return out


@pytest.mark.parametrize("p_on", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("lid", [0, 2])
@pytest.mark.parametrize("m", [40, 32, 1])
def test_eight_row_waves_are_bit_identical_to_four(cuda, m, lid, p_on):
    fd = _fused(cuda)
    a = _run(cuda, fd, lid, m, p_on, 4)
    b = _run(cuda, fd, lid, m, p_on, 8)
    assert a.keys() == b.keys()
    assert len([n for n in a if n.startswith("d ")]) >= 40          # every parameter of the layer got a gradient
    bad = []
    for n in a:
        if n in ("save slots", "gradient workspace"):                # raw bytes (NaN fill included)
            if not torch.equal(a[n], b[n]):
                bad.append((n, int((a[n] != b[n]).sum())))
            continue
        assert bool(torch.isfinite(a[n].float()).all()), n
        if not torch.equal(a[n], b[n]):
            bad.append((n, float((a[n].float() - b[n].float()).abs().max())))
    assert not bad, bad
