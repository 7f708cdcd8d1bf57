"""FP8 (e4m3) inference without a GPU: the reference quantiser on hand-picked values, the scale formulas, which layers of the SUN RGB-D
and KITTI models take the fp8 route, the host-only launch plan, the errors, and the new prototypes in the header-derived binding."""
import copy
import ctypes as C
import math

import pytest
import torch

import projects.mmdet3d_plugin  # noqa: F401
from fp8_ref import exponent_ref, lut, quant_ref
from uni3detr_amd import abi
from uni3detr_amd import native as nv
from uni3detr_amd.inference import InferenceModel, classify, classify_fp8, fp8_exponent

NEW = ("u3d_quant_rows_e4m3", "u3d_absmax_rows", "u3d_bn_fold_fp8_job_bytes", "u3d_bn_fold_fp8_batched", "u3d_igemm_fwd_affine_fp8",
       "u3d_igemm_fwd_fp8_plan")


def _codes(values, e=0):
    return quant_ref(torch.tensor(values, dtype=torch.float32), e)


def test_reference_quantiser_on_hand_picked_values():
    c, nan = _codes([0.0, -0.0, 448.0, 449.0, 1e4, float("inf"), float("-inf"), float("nan"), 2.0 ** -9, 2.0 ** -10, -448.0])
    assert c[:7].tolist() == [0x00, 0x80, 0x7e, 0x7e, 0x7e, 0x7e, 0xfe] and c[10].item() == 0xfe
    assert nan.tolist() == [False] * 7 + [True] + [False] * 3 and (c[7].item() & 0x7f) == 0x7f
    assert c[8].item() == 0x01 and c[9].item() == 0x00                   # the subnormal step 2^-9; half of it ties to even = 0
    # ties to even, normal range: between 1.0 (0x38) and 1.125 (0x39) -> 1.0; between 1.125 and 1.25 (0x3a) -> 1.25
    c, _ = _codes([1.0625, 1.1875, 1.0626, -1.0625, 3 * 2.0 ** -10, 464.0, 463.0])
    assert c.tolist() == [0x38, 0x3a, 0x39, 0xb8, 0x02, 0x7e, 0x7e]      # 1.5 subnormal steps -> 2 (even); 464 would round to NaN unclamped
    # the scale: q(x, e) = q(x * 2^-e, 0), and every code times its scale is what the table says
    c, _ = _codes([448.0 * 32, 3.0, 2.0 ** -4], 5)
    assert c.tolist() == [0x7e, _codes([3.0 / 32])[0].item(), _codes([2.0 ** -9])[0].item()]
    t = lut()
    assert t[0x7e].item() == 448.0 and t[0x01].item() == 2.0 ** -9 and t[0x08].item() == 2.0 ** -6 and math.isnan(t[0x7f].item())


def test_scale_exponents_are_the_smallest_that_fit():
    gen = torch.Generator().manual_seed(5)
    xs = [448.0, 449.0, 224.0, 224.5, 447.99, 1.0, 3.5, 3.5000001, 7e-5, 1e4, 2.0 ** -20 * 448, 896.0] + (torch.rand(200, generator=gen) * 2000).tolist()
    for x in xs:
        for headroom in (1.0, 2.0, 3.0):
            e = fp8_exponent(x * headroom)
            assert e == exponent_ref(x * headroom)
            assert x * headroom <= 448.0 * 2.0 ** e and x * headroom > 448.0 * 2.0 ** (e - 1), (x, headroom, e)
    assert fp8_exponent(0.0) == 0 and fp8_exponent(448.0) == 0 and fp8_exponent(448.0 * 2) == 1 and fp8_exponent(450.0) == 1
    for bad in (float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError):
            fp8_exponent(bad)


def _model(cfg):
    from uni3detr_amd.registry import build_model
    torch.manual_seed(0)
    return build_model(copy.deepcopy(cfg)).set_precision("bf16").eval()


def test_eligibility_sunrgbd_and_kitti_without_a_device():
    from uni3detr_amd.configs import variants
    for cfg in (variants.sunrgbd, variants.kitti_3classes):
        m = _model(cfg)
        fp8, skipped = classify_fp8(m)
        folded = [p[0] for p in classify(m)[0]]
        assert sorted(fp8 + [n for n, _ in skipped]) == sorted(folded) and not set(fp8) & {n for n, _ in skipped}
        # the plan serves every default-fold pair of SECOND3D and the FPN in these models (channel counts % 128 == 0); the route takes
        # those that measured faster than bf16: the 256 -> 128 first conv, the stride-1 256- and 512-channel convs, the FPN's extra convs
        assert fp8 == (["pts_backbone.blocks.0.0"] + [f"pts_backbone.blocks.{b}.{j}" for b in (1, 2) for j in (3, 6, 9, 12, 15)]
                       + [f"pts_neck.extra_blocks.{j}" for j in (0, 3, 6)])
        why = dict(skipped)
        assert all("SparseEncoderHD" in why[n] for n in folded if n.startswith("pts_middle_encoder."))
        assert all("128 -> 128" in why[f"pts_backbone.blocks.0.{j}"] and "ms" in why[f"pts_backbone.blocks.0.{j}"] for j in (3, 6, 9, 12, 15))
        assert "stride 2" in why["pts_backbone.blocks.1.0"] and "stride 4" in why["pts_backbone.blocks.2.0"]
        assert "1 x 1 x 1" in why["pts_neck.deblocks.0.0"] and len(skipped) == 2 + 5 + 2 + 1
        inf = InferenceModel(m, dense_fp8=True)
        assert inf.fp8_layers == fp8 and inf.fp8_skipped == skipped and inf.folded == folded
        off = InferenceModel(m)
        assert off.fp8_layers == [] and off.fp8_skipped == [] and not off.dense_fp8
    # a layer the plan does not serve is skipped with the shape in the reason
    m.pts_backbone.blocks[0][3].weight = torch.nn.Parameter(torch.zeros(128, 64, 1, 3, 3))
    m.pts_backbone.blocks[0][3].in_channels = 64
    fp8, skipped = classify_fp8(m)
    assert "pts_backbone.blocks.0.3" not in fp8 and "64 -> 128" in dict(skipped)["pts_backbone.blocks.0.3"]


def test_plan_query_is_host_only_and_names_what_it_serves():
    for n in (300, 700, 48000, 192000):
        for cin, cout in ((128, 128), (256, 128), (128, 256), (256, 256), (512, 512)):
            p = nv.fwd_fp8_plan(n, cin, cout, 27, True)
            assert p is not None and p.kernel in ("fp8_glds8_256x256", "fp8_glds8_192x256") and p.cols == 256
            assert p.rows == int(p.kernel.split("_")[2].split("x")[0])
            assert nv.fwd_fp8_plan(n, cin, cout, 1, False) == nv.FwdFp8Plan("fp8_glds8_256x256_rows", 256, 256)
    # 192-row tiles where they finish sooner on 256 CUs: the rule of the bf16 kernels (48 000 rows x 256 columns: 188 -> 250 workgroups)
    assert nv.fwd_fp8_plan(48000, 256, 256, 27, True).rows == 192 and nv.fwd_fp8_plan(192000, 256, 256, 27, True).rows == 256
    for shape in ((300, 64, 128, 27, True), (300, 128, 192, 27, True), (300, 192, 128, 27, True), (300, 128, 64, 9, True),
                  (300, 128, 128, 27, False), (300, 128, 128, 1, True), (0, 128, 128, 27, True), (300, 0, 128, 27, True)):
        assert nv.fwd_fp8_plan(*shape) is None, shape
    # a separate entry: the bf16 plan and its epilogue kinds are what they were
    assert sorted(nv.FWD_EPI) == ["add", "affine", "plain", "stats"]


def test_errors_before_calibration_precision_training():
    from uni3detr_amd.configs import variants
    m = _model(variants.sunrgbd)
    inf = InferenceModel(m, dense_fp8=True)
    assert inf.fp8_layers and not inf.fp8_calibrated
    with torch.no_grad(), pytest.raises(RuntimeError, match="calibrate"):
        with inf.scope():
            pass
    with pytest.raises(RuntimeError, match="calibrate"):
        inf.extract_pts_feat([torch.zeros(10, 6)])
    with pytest.raises(RuntimeError, match="not calibrated"):
        inf.fp8_state()
    with pytest.raises(ValueError, match="layers"):
        inf.load_fp8_state({"headroom": 2.0, "e_a": {"nope": 0}})
    with pytest.raises(RuntimeError, match="dense_fp8"):
        InferenceModel(m).calibrate([])
    for mode in ("fp32", "mixed"):
        with pytest.raises(ValueError, match="bf16"):
            InferenceModel(copy.deepcopy(m).set_precision(mode), dense_fp8=True)
    with pytest.raises(RuntimeError, match="eval"):
        InferenceModel(copy.deepcopy(m).train(), dense_fp8=True)


def test_new_prototypes_are_parsed_and_bound():
    P, I, L = C.c_void_p, C.c_int32, C.c_int64
    p = abi.load().prototypes
    raw = C.CDLL(nv.LIB_PATH)
    for name in NEW:
        assert name in p and name in nv.exported_symbols() and hasattr(raw, name), name
    assert p["u3d_quant_rows_e4m3"] == (I, [P, P, P, I, I, P, P])
    assert p["u3d_absmax_rows"] == (I, [P, P, I, I, P, P])
    assert p["u3d_bn_fold_fp8_batched"] == (I, [P, I, I, P]) and p["u3d_bn_fold_fp8_job_bytes"] == (L, [])
    # u3d_igemm_fwd_affine_bf16's arguments plus the per-column scale in front of the shift
    old, new = p["u3d_igemm_fwd_affine_bf16"][1], p["u3d_igemm_fwd_affine_fp8"][1]
    assert new == old[:4] + [P] + old[4:]
    assert p["u3d_igemm_fwd_fp8_plan"] == (I, [I] * 5 + [P] * 3)
    assert int(nv.lib().u3d_bn_fold_fp8_job_bytes()) == C.sizeof(nv.BnFoldFp8Job) == 112
    assert nv.FWD_FP8_KERNELS == ("fp8_glds8_256x256", "fp8_glds8_192x256", "fp8_glds8_256x256_rows")


HOST_WALK = r"""
#include "fp8_quant.h"
extern "C" void walk(const float* x, unsigned char* q, long n) {
  for (long i = 0; i < n; ++i) q[i] = (unsigned char)u3d_e4m3_from_f32(x[i]);
}
"""


def test_device_quantiser_source_on_the_host_against_torch(tmp_path):
    """csrc/fp8_quant.h is the quantiser the kernels compile; it is plain integer code, so the host compiles it too: every bf16 bit
    pattern under the scales 2^3, 1, 2^-5, and 200 000 random f32 values, against the reference - bit for bit where that is not NaN."""
    import subprocess
    import numpy as np
    from uni3detr_amd import build
    src, so = tmp_path / "walk.cpp", tmp_path / "walk.so"
    src.write_text(HOST_WALK)
    subprocess.run([build.HIPCC, "-x", "c++", "-O1", "-shared", "-fPIC", "-I" + build.CSRC, str(src), "-o", str(so)], check=True, capture_output=True)
    walk = C.CDLL(str(so)).walk
    walk.argtypes, walk.restype = [C.c_void_p, C.c_void_p, C.c_long], None
    bf = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).float()
    gen = torch.Generator().manual_seed(9)
    rnd = torch.randn(200000, generator=gen) * torch.exp2(torch.randint(-14, 11, (200000,), generator=gen).float())
    for x in (bf * 8.0, bf, bf / 32.0, rnd):
        x = x.contiguous()
        got = np.empty(x.numel(), np.uint8)
        walk(x.data_ptr(), got.ctypes.data, x.numel())
        ref, nan = quant_ref(x, 0)
        got = torch.from_numpy(got)
        assert torch.equal(got[~nan], ref[~nan]) and bool(((got[nan] & 0x7f) == 0x7f).all())
