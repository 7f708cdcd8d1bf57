"""NumPy restatement of u3d_scatter_mean_exact (include/u3d_hip.h) and of the spare-row contract of u3d_voxelize_dynamic, shared by
tests/test_dynvox_cpu.py and tests/test_dynvox_gpu.py.  Nothing here touches a device."""
import copy
import math

import numpy as np


def tiny_scannet_large_cfg():
    """ScanNet-large (dynamic voxelization + DynamicSimpleVFE) with two layers per SECOND3D block and one extra FPN conv."""
    from uni3detr_amd.configs import variants
    cfg = copy.deepcopy(variants.scannet_large)
    cfg["pts_backbone"]["layer_nums"] = [2, 2, 2]
    cfg["pts_neck"]["extra_conv"]["num_conv"] = 1
    return cfg


def shift_of(n_total):
    """min(40, 61 - ceil(log2(n_total))): n_total values below 2^(e+1), scaled by 2^(shift - e), sum to less than 2^62."""
    lg = 0
    while (1 << lg) < int(n_total):
        lg += 1
    return min(40, 61 - lg)


def _exponent(max_bits):
    """Unbiased exponent of the largest |v| of a cell from its bit pattern; a subnormal (or zero) maximum counts as 2^-126."""
    return np.maximum(max_bits >> 23, 1).astype(np.int64) - 127


def quantised_sums(points, rank, n_voxels):
    """-> (acc: Python-int sums [V, F] as an object array, e int64 [V, F], counts int32 [V], shift): passes 1 and 2."""
    points = np.ascontiguousarray(points, np.float32)
    n, nfeat = points.shape
    shift = shift_of(n)
    live = (rank >= 0) & (rank < n_voxels)
    bits = points.view(np.uint32) & np.uint32(0x7FFFFFFF)
    max_bits = np.zeros((n_voxels, nfeat), np.uint32)
    np.maximum.at(max_bits, rank[live], bits[live])
    e = _exponent(max_bits)
    counts = np.bincount(rank[live], minlength=n_voxels).astype(np.int32)
    q = np.rint(np.ldexp(points[live].astype(np.float64), (shift - e[rank[live]]).astype(np.int32)))      # power-of-two scale: exact
    assert np.abs(q).max(initial=0.0) <= 2.0 ** (shift + 1)
    acc = np.zeros((n_voxels, nfeat), object)
    for r, row in zip(rank[live].tolist(), q.astype(np.int64).tolist()):           # exact integers, any order
        for f, v in enumerate(row):
            acc[r, f] += v
    return acc, e, counts, shift


def scatter_mean_exact(points, rank, n_voxels):
    """-> (mean f32 [V, F], counts int32 [V]): pass 3 on the sums above - scaled back and divided in float64, rounded once to f32."""
    acc, e, counts, shift = quantised_sums(points, rank, n_voxels)
    assert all(abs(int(a)) < 2 ** 62 for a in acc.reshape(-1))
    total = np.ldexp(np.array(acc.tolist(), np.int64).reshape(acc.shape).astype(np.float64), (e - shift).astype(np.int32))
    mean = np.where(counts[:, None] > 0, total / np.maximum(counts, 1)[:, None], 0.0)
    return mean.astype(np.float32), counts


def mean_f64(points, rank, n_voxels):
    """-> (m float64 [V, F] the exact mean (0 for an empty row), largest |v| per cell float64 [V, F], counts)."""
    points = np.asarray(points, np.float32).astype(np.float64)
    live = (rank >= 0) & (rank < n_voxels)
    nfeat = points.shape[1]
    total, big = np.zeros((n_voxels, nfeat)), np.zeros((n_voxels, nfeat))
    for f in range(nfeat):
        for r in range(n_voxels):
            v = points[live & (rank == r), f]
            if v.size:
                total[r, f] = math.fsum(v.tolist())            # correctly rounded float64 sum
                big[r, f] = np.abs(v).max()
    counts = np.bincount(rank[live], minlength=n_voxels)
    return total / np.maximum(counts, 1)[:, None], big, counts.astype(np.int32)


def bound(m, big, shift):
    """The header's accuracy bound per cell: 2^-23 |m| + 2^-shift max|v_i|."""
    return 2.0 ** -23 * np.abs(m) + 2.0 ** -shift * big


def voxelize_dynamic_spare_rows(coors_exact, n_total):
    """What a capacity-sized call returns given the exact-size call's rows: those rows, then (-1, -1, -1, -1) for every spare row."""
    out = np.full((n_total, 4), -1, np.int32)
    out[:coors_exact.shape[0]] = coors_exact
    return out
