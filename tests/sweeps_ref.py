"""NumPy restatement of upstream mmdet3d LoadPointsFromMultiSweeps, ObjectNameFilter and the sweep choice rule (v1.0.0rc5, recalled;
mmdet3d is not vendored, the semantics in INTEGRATION.md section H are the contract), written loop by loop.  `explicit=True` replaces
upstream's `xyz @ R.T` (BLAS, summation order unpinned) by the fixed order the device uses, (r0*x + r1*y) + r2*z in float64, so the
device result can be compared bit for bit.  Used by test_sweeps_cpu.py and test_sweeps_gpu.py."""
import numpy as np


def choose(n_sweeps, sweeps_num, test_mode=False, rng=np.random):
    if n_sweeps <= sweeps_num:
        return np.arange(n_sweeps)
    if test_mode:
        return np.arange(sweeps_num)
    return rng.choice(n_sweeps, sweeps_num, replace=False)


def remove_close(points, radius=1.0):
    x_filt = np.abs(points[:, 0]) < radius
    y_filt = np.abs(points[:, 1]) < radius
    not_close = np.logical_not(np.logical_and(x_filt, y_filt))
    return points[not_close]


def rotate_translate(xyz, rot, trans, explicit=False):
    """float32 [n, 3] -> float32 [n, 3]: `xyz @ R.T` rounded to float32, then `+= t` in float64, rounded again."""
    xyz = np.asarray(xyz, np.float32)
    rot, trans = np.asarray(rot, np.float64), np.asarray(trans, np.float64)
    if explicit:
        x, y, z = (xyz[:, k].astype(np.float64) for k in range(3))
        r = np.stack([((rot[i, 0] * x + rot[i, 1] * y) + rot[i, 2] * z).astype(np.float32) for i in range(3)], 1)
    else:
        r = np.empty_like(xyz)
        r[:] = xyz @ rot.T
    r += trans                                   # float32 += float64: computed in float64, rounded to float32
    return r


def load_points_from_multi_sweeps(key_points, sweeps, timestamp, sweeps_num=10, load_dim=5, use_dim=(0, 1, 2, 4), pad_empty_sweeps=False,
                                  remove_close_=False, test_mode=False, rng=np.random, choices=None, explicit=False, read=None):
    """One scene: key_points float32 [n, load_dim]; sweeps: the info's sweep dicts (data_path, timestamp in microseconds,
    sensor2lidar_rotation / _translation); timestamp: the key frame's, in seconds.  read(path) -> float32 array (default np.fromfile).
    -> (points float32 [m, len(use_dim)], choices)."""
    read = read or (lambda path: np.fromfile(path, dtype=np.float32))
    points = np.array(key_points, np.float32, copy=True)
    points[:, 4] = 0
    sweep_points_list = [points]
    ts = timestamp
    if pad_empty_sweeps and len(sweeps) == 0:
        choices = np.zeros(0, np.int64)
        for i in range(sweeps_num):
            if remove_close_:
                sweep_points_list.append(remove_close(points))
            else:
                sweep_points_list.append(points)
    else:
        if choices is None:
            choices = choose(len(sweeps), sweeps_num, test_mode, rng)
        for idx in choices:
            sweep = sweeps[idx]
            points_sweep = read(sweep["data_path"])
            points_sweep = np.copy(points_sweep).reshape(-1, load_dim)
            if remove_close_:
                points_sweep = remove_close(points_sweep)
            sweep_ts = sweep["timestamp"] / 1e6
            points_sweep[:, :3] = rotate_translate(points_sweep[:, :3], sweep["sensor2lidar_rotation"], sweep["sensor2lidar_translation"],
                                                   explicit)
            points_sweep[:, 4] = ts - sweep_ts
            sweep_points_list.append(points_sweep)
    points = np.concatenate(sweep_points_list, 0)
    points = points[:, list(use_dim)]
    return points, np.asarray(choices, np.int64)


def object_name_filter(gt_bboxes_3d, gt_labels_3d, classes):
    labels = list(range(len(classes)))
    gt_bboxes_mask = np.array([n in labels for n in gt_labels_3d], dtype=np.bool_)
    return gt_bboxes_3d[gt_bboxes_mask], gt_labels_3d[gt_bboxes_mask]


M32 = 0xFFFFFFFF


def mix32(x):
    """datapath.hip dp_mix on uint32."""
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def shuffle_key(seed, scene):
    """the key k_point_shuffle derives from the 64-bit device seed for scene `scene`."""
    seed &= (1 << 64) - 1
    return mix32((seed & M32) ^ mix32(((seed >> 32) + 0x85ebca6b * (scene + 1)) & M32) ^ 0x27d4eb2f)


def feistel_perm(i, n, key):
    """uni3detr_amd/csrc/datapath.hip dp_perm, in Python integers (uint32 wrap-around): the keyed permutation of PointShuffle."""
    bits = 2
    while (1 << bits) < n:
        bits += 1
    if bits & 1:
        bits += 1
    half = bits >> 1
    mask = (1 << half) - 1
    x = i
    while True:
        l, r = x >> half, x & mask
        for rd in range(4):
            f = mix32(r ^ ((key + 0x9E3779B9 * (rd + 1)) & M32)) & mask
            l, r = r, l ^ f
        x = (l << half) | r
        if x < n:
            return x
