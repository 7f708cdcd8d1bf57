"""Eval-mode BatchNorm folding without a GPU: InferenceModel's layer classification and refusals, the job table of
u3d_bn_fold_batched, the header / binding pair of the new entries, the launch plan of u3d_igemm_fwd_affine_bf16, and a numpy
restatement of the fold kernel's f32 arithmetic that justifies the GPU test's "at most 1 % of the elements differ" cap."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import projects.mmdet3d_plugin  # noqa: F401
from uni3detr_amd import native as nv
from uni3detr_amd.inference import InferenceModel, classify

NEW = ("u3d_bn_fold_job_bytes", "u3d_bn_fold_job_blocks", "u3d_bn_fold_batched", "u3d_igemm_fwd_affine_bf16", "u3d_igemm_fwd_plan")


def tiny_cfg():
    """The SUN RGB-D model with two layers per SECOND3D block and one extra FPN conv: every kind of layer, a quarter of the parameters."""
    from uni3detr_amd.configs.sunrgbd import model as MODEL_CFG
    cfg = copy.deepcopy(MODEL_CFG)
    cfg["pts_backbone"]["layer_nums"] = [2, 2, 2]
    cfg["pts_neck"]["extra_conv"]["num_conv"] = 1
    return cfg


@pytest.fixture(scope="module")
def model():
    from uni3detr_amd.registry import build_model
    torch.manual_seed(0)
    return build_model(tiny_cfg())


def test_new_symbols_are_declared_and_bound():
    lib = ctypes.CDLL(nv.LIB_PATH)
    for name in NEW:
        assert name in nv.exported_symbols(), name            # = declared in include/u3d_hip.h (tests/test_abi_cpu.py)
        assert hasattr(lib, name), name
    # the record the kernel reads and the one the host fills are the same bytes
    assert int(nv.lib().u3d_bn_fold_job_bytes()) == ctypes.sizeof(nv.BnFoldJob) == 104


def test_classification_names_every_conv_bn_pair_once(model):
    m = copy.deepcopy(model).set_precision("bf16").eval()
    inf = InferenceModel(m)
    folded, unfolded = inf.folded, dict(inf.unfolded)
    assert len(inf.unfolded) == len(unfolded) and not set(folded) & set(unfolded)
    # SECOND3D: all 3 x (1 + 2) convs; FPN: the plain-conv first level and the extra conv; encoder: the strided 64 -> 128 conv, conv_out
    assert folded == (["pts_middle_encoder.encoder_layers.encoder_layer3.2.0", "pts_middle_encoder.conv_out.0"]
                      + [f"pts_backbone.blocks.{b}.{j}" for b in range(3) for j in (0, 3, 6)]
                      + ["pts_neck.deblocks.0.0", "pts_neck.extra_blocks.0"])
    assert "conv_input" in unfolded["pts_middle_encoder.conv_input.0"]
    for lvl, blocks in (("1", 2), ("2", 2)):
        for b in range(blocks):
            for c in ("conv1", "conv2"):
                assert "narrow" in unfolded[f"pts_middle_encoder.encoder_layers.encoder_layer{lvl}.{b}.{c}"]
        assert "narrow" in unfolded[f"pts_middle_encoder.encoder_layers.encoder_layer{lvl}.2.0"]
    for lvl in ("3", "4"):
        for b in range(2):
            for c in ("conv1", "conv2"):
                assert "halo" in unfolded[f"pts_middle_encoder.encoder_layers.encoder_layer{lvl}.{b}.{c}"]
    for i in (1, 2):
        assert "transposed" in unfolded[f"pts_neck.deblocks.{i}.0"]
    # every BatchNorm of the feature extractor is accounted for, once
    n_bn = sum(isinstance(x, torch.nn.modules.batchnorm._BatchNorm) for x in m.modules())
    assert len(folded) + len(unfolded) == n_bn
    # classify() alone gives the same answer and hands out the parameters the fold reads
    f2, u2 = classify(m)
    assert [p[0] for p in f2] == folded and u2 == inf.unfolded
    mods = dict(m.named_modules())
    for name, w, layout, bn in f2:
        assert w is mods[name].weight and layout == ("dhwio" if name.startswith("pts_middle_encoder") else "oidhw")
        assert bn.num_features == nv.conv_weight_strides(tuple(w.shape), layout)[1]


def test_refuses_training_mode_other_precisions_and_gradients(model):
    m = copy.deepcopy(model)
    with pytest.raises(RuntimeError, match="eval"):
        InferenceModel(m.set_precision("bf16").train())
    m.eval()
    for mode in ("fp32", "mixed", "parity"):
        with pytest.raises(ValueError, match="bf16"):
            InferenceModel(m.set_precision(mode))
    fresh = copy.deepcopy(model).eval()                       # set_precision never called: fp32 storage
    with pytest.raises(ValueError, match="bf16"):
        InferenceModel(fresh)
    inf = InferenceModel(m.set_precision("bf16"))
    assert torch.is_grad_enabled()
    with pytest.raises(RuntimeError, match="gradients"):
        with inf.scope():
            pass
    m.train()
    with torch.no_grad(), pytest.raises(RuntimeError, match="training"):
        with inf.scope():
            pass


def test_model_without_inference_model_is_untouched(model):
    """The folded route exists only inside a scope: nothing is installed on the model or left behind in sparse.py."""
    from uni3detr_amd import sparse as sp
    m = copy.deepcopy(model).set_precision("bf16").eval()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    inf = InferenceModel(m)
    assert sp._FOLD[0] is None
    with torch.no_grad(), pytest.raises(RuntimeError, match="device"):       # a CPU model has no folded buffers: refused, and ...
        with inf.scope():
            pass
    assert sp._FOLD[0] is None                                               # ... the scope is not left open
    after = m.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)


def test_job_table_strides_for_both_layouts_and_monotone_first_block():
    # element (k, co, ci) of the master weight, through the strides the table carries, for both checkpoint layouts
    for layout, shape in (("dhwio", (1, 3, 3, 8, 12)), ("oidhw", (12, 8, 1, 3, 3)), ("oidhw", (20, 4, 1, 1, 1)), ("dhwio", (3, 3, 3, 64, 64))):
        w = torch.arange(int(np.prod(shape)), dtype=torch.float32).view(shape)
        k, cout, cin, sk, sa, sb = nv.conv_weight_strides(shape, layout)
        koi = (w.reshape(k, cin, cout).permute(0, 2, 1) if layout == "dhwio" else w.reshape(cout, cin, k).permute(2, 0, 1))
        flat = w.reshape(-1)
        for kk, co, ci in ((0, 0, 0), (k - 1, cout - 1, cin - 1), (k // 2, 1, 2), (0, cout - 1, 0)):
            assert flat[kk * sk + co * sa + ci * sb] == koi[kk, co, ci], (layout, shape)
    with pytest.raises(ValueError):
        nv.conv_weight_strides((1, 1, 1, 4, 4), "iodhw")

    shapes = [("dhwio", (1, 3, 3, 128, 128)), ("oidhw", (64, 64, 3, 3, 3)), ("oidhw", (256, 128, 1, 1, 1)), ("dhwio", (1, 1, 5, 36, 20)),
              ("dhwio", (1, 1, 3, 8, 12))]
    specs = [dict(w=1000 + i, gamma=2000 + i, beta=3000 + i, mean=4000 + i, var=5000 + i, w_folded=6000 + i,
                  shift=None if i == 1 else 7000 + i, shape=s, layout=lay, eps=1e-3, scale_only=i == 1)
             for i, (lay, s) in enumerate(shapes)]
    jobs, total = nv.bn_fold_job_table(specs)
    assert len(jobs) == 5
    fb = [j.first_block for j in jobs]
    assert fb[0] == 0 and all(b > a for a, b in zip(fb, fb[1:]))          # strictly ascending: every job owns at least one block
    counts = [j.kvol * j.cout * j.cin for j in jobs]
    assert counts == [9 * 128 * 128, 27 * 64 * 64, 128 * 256, 5 * 36 * 20, 3 * 8 * 12]
    per_block = 2048
    blocks = [-(-c // per_block) for c in counts]
    assert [int(nv.lib().u3d_bn_fold_job_blocks(j.kvol, j.cout, j.cin)) for j in jobs] == blocks
    assert fb == [sum(blocks[:i]) for i in range(5)] and total == sum(blocks)
    assert counts[3] % per_block != 0                                     # the ragged job of the GPU test
    assert [(j.sk, j.sa, j.sb) for j in jobs[:3]] == [(128 * 128, 1, 128), (1, 64 * 27, 27), (1, 128, 1)]
    assert [j.scale_only for j in jobs] == [0, 1, 0, 0, 0] and jobs[1].shift is None and jobs[2].shift == 7002
    assert abs(jobs[0].eps - 1e-3) < 1e-9 and jobs[4].w == 1004 and jobs[4].w_folded == 6004
    bad = dict(specs[0], shape=(1, 1, 1, 6, 8))
    with pytest.raises(nv.U3DError, match="multiple of 4"):
        nv.bn_fold_job_table([bad])
    with pytest.raises(nv.U3DError, match="shift"):
        nv.bn_fold_job_table([dict(specs[0], shift=None)])


# (n, cin, cout, kvol, table) -> the kernel family the affine launch takes: the shapes of tests/test_bn_fold_gpu.py, one per kernel
AFFINE_PLAN = [
    ((300, 128, 128, 9, True), ("glds_128x128",)),
    ((300, 128, 64, 9, True), ("glds_128x64",)),
    ((32768 + 37, 256, 256, 27, True), ("glds8_256x256", "glds8_192x256")),
    ((40960 + 5, 128, 128, 27, True), ("glds8_256x128", "glds8_192x128")),
    ((32768 + 37, 128, 256, 1, False), ("glds_256x256",)),
]


@pytest.mark.parametrize("shape,family", AFFINE_PLAN)
def test_affine_plan_reaches_every_kernel_family(shape, family):
    name, rows, cols = nv.igemm_fwd_affine_plan(*shape)
    assert name in family
    assert (rows, cols) == tuple(int(v) for v in name.split("_")[1].split("x"))
    # wherever the statistics entry runs on an LDS-DMA kernel it is the same one: one row tile per partial
    assert nv.fwd_stats_layout(*shape)[1] == rows


def test_affine_plan_never_takes_a_direct_operand_kernel():
    # shapes the direct-operand kernels serve for the plain forward: not multiples of 64, so the affine entry serves none of them
    for cin, cout in ((16, 16), (32, 32), (16, 32), (32, 64)):
        assert nv.igemm_fwd_affine_plan(50000, cin, cout, 27, True) is None
    # 64 -> 64 with 27 offsets: whatever the plain forward takes, the affine launch is an LDS-DMA tile
    assert nv.igemm_fwd_affine_plan(50000, 64, 64, 27, True)[0].startswith("glds")


def _bf16_bits_rne_f32(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def bf16_bits_from_f64(v):
    """bf16 bit patterns of float64 values rounded ONCE (nearest, ties to even): the candidates are the bf16 numbers around the
    f32-rounded value, the nearest in float64 wins."""
    v = np.asarray(v, np.float64)
    base = (v.astype(np.float32).view(np.uint32) >> 16).astype(np.int64)
    cand = np.stack([base - 1, base, base + 1])                                      # neighbours in magnitude order, same sign
    vals = (cand.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    d = np.abs(vals - v[None])
    best = d.min(0)
    tie = (d == best[None])
    pick_even = tie & ((cand & 1) == 0)
    choose = np.where(pick_even.any(0), pick_even.argmax(0), tie.argmax(0))
    return np.take_along_axis(cand, choose[None], 0)[0].astype(np.uint16)


def test_f32_fold_arithmetic_rarely_differs_from_direct_rounding():
    """The kernel computes scale and w * scale in f32 and rounds to bf16; the GPU test compares with bf16(w * scale in float64) and
    allows 1 % of the elements to differ (by one ulp).  With var in [0.5, 2], gamma in [0.5, 1.5], w ~ N(0, 1) the double rounding
    f64 -> f32 -> bf16 moves far fewer: an f32 error of <= 1.5 ulp_f32 (scale's two roundings + the product's) flips the bf16 rounding
    only within that distance of a tie, i.e. for about 2 * 1.5 / 2^16 = 5e-5 of the elements."""
    rng = np.random.default_rng(7)
    cout, cin, k = 128, 128, 9
    w = rng.standard_normal((k, cout, cin)).astype(np.float32)
    var = rng.uniform(0.5, 2.0, cout).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    eps = np.float32(1e-3)
    scale32 = (gamma / np.sqrt(var + eps, dtype=np.float32)).astype(np.float32)
    got = _bf16_bits_rne_f32((w * scale32[None, :, None]).astype(np.float32))
    scale64 = gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + float(eps))
    ref = bf16_bits_from_f64(w.astype(np.float64) * scale64[None, :, None])
    diff = got.astype(np.int32) - ref.astype(np.int32)
    assert np.abs(diff).max() <= 1
    share = float((diff != 0).mean())
    print("share of elements where f32 arithmetic + RNE differs from direct rounding:", share)
    assert share <= 1e-3                                                             # an order of magnitude under the GPU test's cap
    # the helper itself: exact on bf16-representable values and on a value just above / below a tie
    exact = np.array([1.0, -2.5, 0.15625, 3.0e-5], np.float64)
    assert (bf16_bits_from_f64(exact) == _bf16_bits_rne_f32(exact.astype(np.float32))).all()
    tie = 1.0 + 2.0 ** -8                                                            # halfway between bf16(1.0) and the next one
    assert bf16_bits_from_f64(np.array([tie + 1e-12, tie - 1e-12, tie])).tolist() == [0x3F81, 0x3F80, 0x3F80]
