"""GPU: the decoder layers' value-gradient records scattered by one call (u3d_value_scatter_layers, fused_decoder.ONE_SCATTER) against
the route it replaces: one u3d_value_scatter call per layer into a zeroed f32 volume, cast to bf16 afterwards.  Per cell both add
the same f32 layer sums, formed in the same order, to +0.0f in the same order and round once - the bits must be equal, the sign of
zero and the cells nobody touches included."""
import pytest
import torch

import projects.mmdet3d_plugin  # noqa: F401
from uni3detr_amd import native as nv
from uni3detr_amd.configs.sunrgbd import model as MODEL_CFG
from uni3detr_amd.registry import build_model

pytestmark = pytest.mark.gpu

N_CELLS, M = 240, 16
ALL3, LAST_ONLY, CROWDED, NEG_ZERO = 5, 9, 17, 33


def _layers():
    """Three layers of 16 rows (128 entries each): seeded d(sample) rows and corner weights, hand-built corner cells."""
    g = torch.Generator(device="cpu").manual_seed(23)
    out = []
    for l in range(3):
        ds = torch.randn(M, 256, generator=g)
        w = torch.rand(M, 8, generator=g)
        cell = torch.randint(40, N_CELLS, (M, 8), generator=g, dtype=torch.int32)      # the rest: random cells, some shared
        cell[0, 0] = ALL3                                     # (1) a cell every layer hits
        cell[1, 3] = ALL3
        cell[2, :4] = torch.tensor([-1, N_CELLS, 1000, -7])   # (4) ids outside the volume are ignored
        out.append([ds, cell, w])
    out[2][1][3, 5] = LAST_ONLY                               # (2) hit only by layer 2 - the one added last in the default order
    out[1][1][4:13, :] = CROWDED                              # (3) 9 rows x 8 corners = 72 entries of ONE layer on one cell: the scan path
    out[0][1][15, 7] = CROWDED                                #     ... which another layer reaches through its id list
    # (5) a cell whose only contribution is exactly -0.0: the exact product -1e-60 is not zero and rounds to -0.0f
    out[0][0][14, :] = 1e-30
    out[0][2][14, :] = -1e-30
    out[0][1][14, :] = -1
    out[0][1][14, 2] = NEG_ZERO
    return out


def _pack(ds, cell, w, dev):
    rec = torch.cat([ds.reshape(-1).view(torch.uint8), cell.reshape(-1).view(torch.uint8), w.reshape(-1).view(torch.uint8)]).to(dev)
    assert rec.numel() == nv.lib().u3d_value_records_bytes(ds.shape[0])
    return rec


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 0, 1), (1, 2, 0)], ids=lambda o: "".join(map(str, o)))
def test_one_call_is_the_f32_accumulator_bit_for_bit(cuda, order):
    layers = _layers()
    assert all(int((layers[l][1] == NEG_ZERO).sum()) == (1 if l == 0 else 0) for l in range(3))
    recs = [_pack(*t, cuda) for t in layers]
    ref = torch.zeros(N_CELLS, 256, dtype=torch.float32, device=cuda)
    for l in order:
        nv.value_scatter(recs[l], M, ref)
    ref = ref.to(torch.bfloat16)
    got = torch.zeros(N_CELLS, 256, dtype=torch.bfloat16, device=cuda)
    nv.value_scatter_layers(recs, [M] * 3, got, order)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    # the cases are what they claim to be
    touched = ref.float().abs().sum(1) > 0
    assert bool(touched[ALL3]) and bool(touched[LAST_ONLY]) and bool(touched[CROWDED]) and not bool(touched[:5].any())
    assert bool((got[NEG_ZERO].view(torch.int16) == 0).all()), "(+0.0) + (-0.0) is +0.0"
    neg = torch.zeros(N_CELLS, 256, dtype=torch.float32, device=cuda)
    neg[NEG_ZERO] = 1.0
    nv.value_scatter(recs[0], M, neg)
    assert bool((neg[NEG_ZERO] == 1.0).all())                  # ... and that layer's sum there was a zero


def test_two_layers_and_a_single_layer(cuda):
    layers = _layers()
    recs = [_pack(*t, cuda) for t in layers]
    for pick in ([1, 0], [2]):
        ref = torch.zeros(N_CELLS, 256, dtype=torch.float32, device=cuda)
        for l in pick:
            nv.value_scatter(recs[l], M, ref)
        got = torch.zeros(N_CELLS, 256, dtype=torch.bfloat16, device=cuda)
        nv.value_scatter_layers([recs[l] for l in pick], [M] * len(pick), got)
        assert torch.equal(got.view(torch.int16), ref.to(torch.bfloat16).view(torch.int16))


def test_entry_return_codes(cuda):
    import ctypes as C
    lib = nv.lib()
    rec = _pack(*_layers()[0], cuda)
    dv = torch.zeros(N_CELLS, 256, dtype=torch.bfloat16, device=cuda)
    wsb = int(lib.u3d_value_scatter_layers_workspace(2, N_CELLS))
    assert wsb == N_CELLS * (1 + 2 * 65) * 4 and lib.u3d_value_scatter_layers_workspace(5, N_CELLS) == 0
    work = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    P = (C.c_void_p * 2)(rec.data_ptr(), rec.data_ptr())
    I = lambda *v: (C.c_int32 * len(v))(*v)
    call = lambda p, m, o, L, ws: lib.u3d_value_scatter_layers(p, m, o, L, N_CELLS, dv.data_ptr(), work.data_ptr(), ws, None)
    assert call(P, I(M, M), I(0, 0), 2, wsb) == -1                      # the order is not a permutation
    assert call(P, I(M, 0), I(0, 1), 2, wsb) == -1                      # a layer without rows
    assert call((C.c_void_p * 2)(rec.data_ptr(), None), I(M, M), I(0, 1), 2, wsb) == -1
    assert call(P, I(M, M), I(0, 1), 5, wsb) == -1
    assert call(P, I(M, M), I(0, 1), 2, wsb - 4) == -4                  # U3D_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((dv.view(torch.int16) == 0).all()), "a refused call must not have launched anything"


def test_fused_decoder_volume_gradient_does_not_depend_on_the_route(cuda, monkeypatch):
    """Three fused decoder layers on a small volume (B = 1, 2 x 300 queries): the gradient w.r.t. the sampled volume with the one scatter
    of the last backward and with one scatter per layer into the f32 accumulator."""
    from uni3detr_amd.plugin import fused_decoder as fdm
    torch.manual_seed(11)
    head = build_model(MODEL_CFG).pts_bbox_head.to(cuda)
    with torch.no_grad():
        for m in head.modules():                       # non-trivial gate and norm parameters, dropout off
            if hasattr(m, "attention_weights"):
                m.attention_weights.weight.normal_(0, 0.05)
                m.attention_weights.bias.normal_(0, 0.5)
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
            if hasattr(m, "attn_drop"):
                m.attn_drop = 0.0
    head.train()
    calls = []
    one, per_layer = nv.value_scatter_layers, nv.value_scatter
    monkeypatch.setattr(nv, "value_scatter_layers", lambda *a, **k: calls.append("layers") or one(*a, **k))
    monkeypatch.setattr(nv, "value_scatter", lambda *a, **k: calls.append("one") or per_layer(*a, **k))
    g = torch.Generator(device="cpu").manual_seed(5)
    feats = torch.randn(1, 256, 15, 40, 40, generator=g).clamp_min(0).to(cuda).to(memory_format=torch.channels_last_3d)
    fps = torch.rand(1, 600, 3, generator=g).to(cuda)
    res = {}
    for flag in (True, False):
        monkeypatch.setattr(fdm, "ONE_SCATTER", flag)
        del calls[:]
        f = feats.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            outs = head(f, None, fps)
        tot = sum((v.float() ** 2).sum() * w for v, w in zip((outs["all_cls_scores"], outs["all_bbox_preds"], outs["all_iou_preds"]), (1.0, 0.1, 1.0)))
        head.zero_grad(set_to_none=True)
        tot.backward()
        assert calls == (["layers"] if flag else ["one"] * 3), calls
        res[flag] = f.grad.clone()
    assert float(res[True].float().abs().sum()) > 0
    assert res[True].dtype == res[False].dtype and res[True].stride() == res[False].stride()
    assert torch.equal(res[True].view(torch.int16) if res[True].dtype == torch.bfloat16 else res[True],
                       res[False].view(torch.int16) if res[False].dtype == torch.bfloat16 else res[False])
