"""InferenceModel(sparse_levels=True) without a GPU: the classification of the sparse encoder's block and strided convolutions for the
tiny, the SUN RGB-D and the ScanNet-large model, the unchanged default, the header / binding pair of the new entries - and a numpy
float64 restatement of the affine epilogue of the halo and direct-operand kernels (shift, then addend, then ReLU, ONE rounding) that
tests/test_bn_fold_sparse_gpu.py measures the kernels against."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import projects.mmdet3d_plugin  # noqa: F401
from test_bn_fold_cpu import bf16_bits_from_f64, tiny_cfg
from uni3detr_amd import native as nv
from uni3detr_amd.inference import InferenceModel, classify

NEW = ("u3d_subm_halo_conv_bf16", "u3d_igemm_direct_affine_bf16")


def affine_epilogue64(acc, shift, addend=None, relu=False):
    """What the affine epilogue computes per output element before its one rounding, in float64: v = acc + shift[col]; v += addend[m][col]
    if there is one; v = max(v, 0) if relu.  acc [n, C] (the convolution with the folded weights), shift [C], addend [n, C]."""
    v = np.asarray(acc, np.float64) + np.asarray(shift, np.float64)[None, :]
    if addend is not None:
        v = v + np.asarray(addend, np.float64)
    if relu:
        v = np.maximum(v, 0.0)
    return v


def affine_epilogue_bf16_bits(acc, shift, addend=None, relu=False):
    """bf16 bit patterns of the epilogue's result: rounded once, nearest-even, from the float64 value."""
    return bf16_bits_from_f64(affine_epilogue64(acc, shift, addend, relu))


def test_epilogue_restatement_order_and_single_rounding():
    acc = np.array([[1.0, -3.0], [0.25, 2.0]])
    shift = np.array([0.5, 1.0])
    add = np.array([[-2.0, 4.0], [1.0, -5.0]])
    # ReLU comes LAST: relu(acc + shift) + addend would keep the negative sums
    assert affine_epilogue64(acc, shift, add, True).tolist() == [[0.0, 2.0], [1.75, 0.0]]
    assert affine_epilogue64(acc, shift, add, False).tolist() == [[-0.5, 2.0], [1.75, -2.0]]
    assert affine_epilogue64(acc, shift, None, True).tolist() == [[1.5, 0.0], [0.75, 3.0]]
    # one rounding: acc + shift rounded to bf16 first (what conv -> bf16 -> BatchNorm does) lands on another bf16 number
    t = 2.0 ** -8                                           # bf16 spacing in [1, 2) is 2^-7
    acc1, sh1, ad1 = np.array([[1.0 + t]]), np.array([0.0]), np.array([[0.75 * t]])
    once = affine_epilogue_bf16_bits(acc1, sh1, ad1)        # 1 + 1.75 t -> 1 + 2 t
    first = bf16_bits_from_f64(acc1)                        # tie -> even: 1.0
    twice = bf16_bits_from_f64((first.astype(np.uint32) << 16).view(np.float32).astype(np.float64) + ad1)      # 1 + 0.75 t -> 1.0
    assert once.tolist() == [[0x3F81]] and twice.tolist() == [[0x3F80]]


def test_new_symbols_are_declared_and_bound():
    lib = ctypes.CDLL(nv.LIB_PATH)
    for name in NEW:
        assert name in nv.exported_symbols() and hasattr(lib, name), name     # exported_symbols() = declared in include/u3d_hip.h
    assert callable(nv.subm_halo_conv_affine) and callable(nv.igemm_direct_affine)


def _cfgs():
    from uni3detr_amd.configs import variants
    return {"tiny": tiny_cfg, "sunrgbd": lambda: copy.deepcopy(variants.sunrgbd), "scannet_large": lambda: copy.deepcopy(variants.scannet_large)}


@pytest.fixture(scope="module", params=["tiny", "sunrgbd", "scannet_large"])
def named_model(request):
    from uni3detr_amd.registry import build_model
    torch.manual_seed(0)
    return request.param, build_model(_cfgs()[request.param]()).set_precision("bf16").eval()


def test_sparse_levels_classification(named_model):
    from uni3detr_amd.plugin.sparse_encoder import SparseBasicBlock
    which, m = named_model
    f0, u0 = classify(m)
    f1, u1 = classify(m, sparse_levels=True)
    d_names, s_names = [p[0] for p in f0], [p[0] for p in f1]
    # unfolded: exactly conv_input + the FPN entries of the default classification, with their reasons
    assert u1 == [(n, why) for n, why in u0 if n == "pts_middle_encoder.conv_input.0" or n.startswith("pts_neck.")]
    assert u1[0][0] == "pts_middle_encoder.conv_input.0" and "conv_input" in u1[0][1]
    # folded: every encoder block conv and strided conv, then conv_out, in forward order, then the default list's dense layers
    enc, blocks, narrow_strided = [], 0, 0
    for si, stage in enumerate(m.pts_middle_encoder.encoder_layers):
        for j, mod in enumerate(stage):
            base = f"pts_middle_encoder.encoder_layers.encoder_layer{si + 1}.{j}"
            if isinstance(mod, SparseBasicBlock):
                enc += [base + ".conv1", base + ".conv2"]
                blocks += 1
            else:
                enc.append(base + ".0")
                narrow_strided += not (mod[0].cin % 64 == 0 and mod[0].cout % 64 == 0)
    enc.append("pts_middle_encoder.conv_out.0")
    assert s_names == enc + [n for n in d_names if not n.startswith("pts_middle_encoder.")]
    assert set(d_names) <= set(s_names)
    order = {n: i for i, (n, _) in enumerate(m.named_modules())}
    assert [order[n] for n in s_names] == sorted(order[n] for n in s_names)
    # the default list plus the blocks' convs and the narrow strided ones; disjoint from `unfolded`; every BatchNorm once
    assert len(s_names) == len(d_names) + 2 * blocks + narrow_strided and len(set(s_names)) == len(s_names)
    assert not set(s_names) & {n for n, _ in u1}
    n_bn = sum(isinstance(x, torch.nn.modules.batchnorm._BatchNorm) for x in m.modules())
    assert len(s_names) + len(u1) == n_bn == len(d_names) + len(u0)
    if which == "sunrgbd":
        assert (len(d_names), len(u0)) == (24, 21) and blocks == 8 and narrow_strided == 2
        assert (len(s_names), len(u1)) == (24 + 16 + 2, 3)
    if which == "tiny":
        assert (len(d_names), len(u0)) == (13, 21)
    # the parameters the fold reads
    mods = dict(m.named_modules())
    for name, w, layout, bn in f1:
        assert w is mods[name].weight and layout == ("dhwio" if name.startswith("pts_middle_encoder") else "oidhw")
        k, cout, cin = nv.conv_weight_strides(tuple(w.shape), layout)[:3]
        assert bn.num_features == cout and cin % 4 == 0


def test_default_is_unchanged_and_wrapper_follows_classify(named_model):
    which, m = named_model
    f0, u0 = classify(m)
    assert classify(m, sparse_levels=False)[1] == u0 and [p[0] for p in classify(m, False)[0]] == [p[0] for p in f0]
    inf = InferenceModel(m)
    assert inf.sparse_levels is False and inf.folded == [p[0] for p in f0] and inf.unfolded == u0
    # the default keeps its reasons for the sparse levels
    why = dict(u0)
    for n, reason in u0:
        if ".conv1" in n or ".conv2" in n:
            assert ("narrow" in reason) or ("halo" in reason), (n, reason)
    assert any("narrow" in r for r in why.values()) and any("halo" in r for r in why.values())
    inf_s = InferenceModel(m, sparse_levels=True)
    f1, u1 = classify(m, sparse_levels=True)
    assert inf_s.sparse_levels is True and inf_s.folded == [p[0] for p in f1] and inf_s.unfolded == u1
    # no device: nothing allocated, the scope refuses
    assert inf_s._by_bn == {} and all(r.w_folded is None and r.route is None for r in inf_s._records)
    with torch.no_grad(), pytest.raises(RuntimeError, match="device"):
        with inf_s.scope():
            pass


def test_halo_condition_is_the_one_the_training_forward_used(monkeypatch):
    """sparse._halo_of against the expression _SparseConv.forward carried before the folded route shared it (there under `nmajor and`):
    every combination of its terms, for a level with and without halo tables."""
    import itertools
    import types
    from uni3detr_amd import sparse as sp
    table = object()
    for subm_halo, rev, halo128, has_level, tab, kv, (cin, cout), n_out in itertools.product(
            (True, False), (True, False), (True, False), (True, False), (table, None), (27, 9),
            ((64, 64), (128, 128), (64, 128), (32, 32), (256, 256)), (4095, 4096)):
        monkeypatch.setattr(sp, "SUBM_HALO", subm_halo)
        monkeypatch.setattr(sp, "REV_SUBM_TABLE", rev)
        monkeypatch.setattr(sp, "HALO_128", halo128)
        level = types.SimpleNamespace(halo=lambda tab=tab: tab) if has_level else None
        geom = types.SimpleNamespace(level=level, n_out=n_out)
        old = bool(sp.SUBM_HALO and sp.REV_SUBM_TABLE and geom.level is not None and kv == 27 and cin == cout
                   and (cin == 64 or (cin == 128 and sp.HALO_128)) and geom.n_out >= 4096
                   and geom.level.halo() is not None)
        got = sp._halo_of(geom, kv, cin, cout)
        assert (got is not None) == old and (got is table if old else got is None)
