"""Dynamic voxelization in the captured inference step, without a GPU: the header / binding pair of the order-free mean, InferenceStep
accepting the ScanNet-large model (and still refusing a dynamic_voxelization flag without a DynamicSimpleVFE) before any device
access, and the NumPy restatement of the fixed-point mean (tests/dynvox_ref.py): permutation invariance and the stated bound."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import projects.mmdet3d_plugin  # noqa: F401
import dynvox_ref as ref
from uni3detr_amd import native as nv
from uni3detr_amd.inference import InferenceModel, InferenceStep

NEW = ("u3d_scatter_mean_exact", "u3d_scatter_mean_exact_workspace")


def test_new_symbols_are_declared_and_bound():
    lib = ctypes.CDLL(nv.LIB_PATH)
    for name in NEW:
        assert name in nv.exported_symbols(), name            # = declared in include/u3d_hip.h (tests/test_abi_cpu.py)
        assert hasattr(lib, name), name
    # per (voxel, feature) one 64-bit sum and one 32-bit maximum; nothing for an empty request
    assert int(nv.lib().u3d_scatter_mean_exact_workspace(37, 3)) == 37 * 3 * 12
    assert int(nv.lib().u3d_scatter_mean_exact_workspace(0, 3)) == 0 and int(nv.lib().u3d_scatter_mean_exact_workspace(37, 0)) == 0
    assert callable(nv.scatter_mean_exact)


def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("device access")
    monkeypatch.setattr(torch.cuda, "current_stream", boom)


def test_step_accepts_the_scannet_large_model_before_any_device_access(monkeypatch):
    from uni3detr_amd.plugin.detector import DynamicSimpleVFE
    from uni3detr_amd.registry import build_model
    torch.manual_seed(0)
    model = build_model(ref.tiny_scannet_large_cfg()).set_precision("bf16").eval()
    assert model.dynamic_voxelization and isinstance(model.pts_voxel_encoder, DynamicSimpleVFE)
    vfe = model.pts_voxel_encoder
    assert (vfe.capacity, vfe.static_eval, vfe.exact_mean) == (None, False, False)         # both routes off until someone turns them on
    _no_device(monkeypatch)
    step = InferenceStep(InferenceModel(model), batch_size=2, point_capacity=1000)
    assert step.feat == int(model.pts_middle_encoder.in_channels) and not hasattr(model.pts_voxel_encoder, "num_features")
    assert (step.batch_size, step.point_capacity, step.fallbacks, step.dynamic) == (2, 1000, 0, True)
    assert step.pts is None and step.n_live is None
    with pytest.raises(RuntimeError, match="capture"):
        step.run([torch.zeros(10, step.feat)])
    step = InferenceStep(InferenceModel(model), batch_size=2, point_capacity=1000, views=2)
    assert step.views == 2 and step.feat == int(model.pts_middle_encoder.in_channels)
    assert (vfe.capacity, vfe.static_eval, vfe.exact_mean) == (None, False, False)         # constructing a step switches nothing


def test_flag_without_a_dynamic_encoder_is_still_refused(monkeypatch):
    from test_bn_fold_cpu import tiny_cfg
    from uni3detr_amd.registry import build_model
    torch.manual_seed(0)
    model = build_model(tiny_cfg()).set_precision("bf16").eval()
    dyn = copy.deepcopy(model)
    dyn.dynamic_voxelization = True                      # the SUN RGB-D model with the flag flipped: no forward exists for it
    _no_device(monkeypatch)
    with pytest.raises(NotImplementedError, match="dynamic_voxelization"):
        InferenceStep(InferenceModel(dyn), batch_size=2, point_capacity=1000)
    assert InferenceStep(InferenceModel(model), batch_size=2, point_capacity=1000).dynamic is False


def _case(seed, n, nfeat, v, mixed=False):
    rng = np.random.default_rng(seed)
    pts = rng.normal(0, 3, (n, nfeat)).astype(np.float32)
    rank = rng.integers(0, v, n).astype(np.int32)
    rank[::8] = -1
    if mixed:                   # magnitudes 1e-3 .. 1e3 and both signs inside voxel 5
        rows = np.flatnonzero(rank == 5)
        pts[rows] = (10.0 ** rng.uniform(-3, 3, (rows.size, nfeat)) * rng.choice([-1.0, 1.0], (rows.size, nfeat))).astype(np.float32)
        pts[rows[0]], pts[rows[1]] = 1e3, -1e-3
    return pts, rank


def test_shift_formula():
    assert [ref.shift_of(n) for n in (0, 1, 2, 4099, 2 ** 21, 2 ** 21 + 1, 2 ** 31 - 1)] == [40, 40, 40, 40, 40, 39, 30]
    for n in (1, 300000, 2 ** 21, 2 ** 25 + 3, 2 ** 31 - 1):
        assert n * 2 ** (ref.shift_of(n) + 1) <= 2 ** 62                                   # n values of at most 2^(shift + 1) each


@pytest.mark.parametrize("mixed", [False, True])
def test_restatement_is_permutation_invariant_and_within_the_bound(mixed):
    n, nfeat, v = 4099, 4, 37
    pts, rank = _case(11, n, nfeat, v, mixed)
    acc, e, counts, shift = ref.quantised_sums(pts, rank, v)
    got, cnt = ref.scatter_mean_exact(pts, rank, v)
    m, big, want_cnt = ref.mean_f64(pts, rank, v)
    assert shift == 40 and np.array_equal(cnt, want_cnt) and np.array_equal(cnt, counts)
    if mixed:
        assert (big[5] == 1e3).all() and cnt[5] > 50               # the 1e3 value next to values down to 1e-3, in one voxel
    err, tol = np.abs(got.astype(np.float64) - m), ref.bound(m, big, shift)
    print(f"mixed={mixed}: largest error / bound {float((err / np.maximum(tol, 1e-300)).max()):.3f}")
    assert (err <= tol).all()
    for seed in (1, 2, 3):
        p = np.random.default_rng(seed).permutation(n)
        acc_p, e_p, counts_p, _ = ref.quantised_sums(pts[p], rank[p], v)
        assert np.array_equal(e_p, e) and np.array_equal(counts_p, counts)
        assert all(int(a) == int(b) for a, b in zip(acc_p.reshape(-1), acc.reshape(-1)))
        got_p, _ = ref.scatter_mean_exact(pts[p], rank[p], v)
        assert np.array_equal(got_p.view(np.uint32), got.view(np.uint32))


def test_restatement_single_points_and_empty_rows():
    rng = np.random.default_rng(5)
    pts = (rng.normal(0, 1, (37, 3)) * 10.0 ** rng.uniform(-3, 3, (37, 3))).astype(np.float32)
    rank = rng.permutation(37).astype(np.int32)
    got, cnt = ref.scatter_mean_exact(pts, rank, 40)
    assert np.array_equal(got[rank].view(np.uint32), pts.view(np.uint32)) and (cnt[rank] == 1).all()
    assert not got[37:].any() and not cnt[37:].any()
    got, cnt = ref.scatter_mean_exact(np.zeros((0, 3), np.float32), np.zeros((0,), np.int32), 4)
    assert got.shape == (4, 3) and not got.any() and not cnt.any()
