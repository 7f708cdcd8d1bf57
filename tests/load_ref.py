"""NumPy restatement of mmdet3d's LoadPointsFromFile and NormalizePointsColor (v1.0.0rc5, recalled from the published behaviour - not in
the reference tree, parity unpinned) under the rule INTEGRATION.md section P declares: the floor of a scene is
np.float32(np.percentile(z.astype(np.float64), 0.99)), i.e. NumPy's `linear` method evaluated in float64 on the exact float32 heights
and rounded once; the height column z - floor32 is computed in float32 and goes in after the third selected column."""
import numpy as np


def read_file(path, load_dim):
    a = np.load(path) if str(path).endswith(".npy") else np.fromfile(str(path), dtype=np.float32)
    return np.asarray(a, np.float32).reshape(-1, load_dim)


def index_and_gamma(n):
    """(i, g) of the `linear` method at q = 0.99 for n values, float64 as NumPy computes them"""
    pos = (n - 1) * np.true_divide(0.99, 100)
    i = np.floor(pos)
    return int(i), float(pos - i)


def floor_by_rule(z):
    """the declared rule spelled out: order statistics, then the two-sided lerp in float64 (no use of np.percentile)"""
    z64 = np.sort(np.asarray(z, np.float32).astype(np.float64))
    n = len(z64)
    if np.isnan(z64).any():
        return np.float64(np.nan)
    i, g = index_and_gamma(n)
    a, b = z64[i], z64[min(i + 1, n - 1)]
    d = b - a
    return a + d * g if g < 0.5 else b - d * (1.0 - g)


def floor_height(z):
    return np.float32(np.percentile(np.asarray(z, np.float32).astype(np.float64), 0.99))


def load_points(raw, use_dim, shift_height=False):
    """raw float32 [n, load_dim] -> (points [n, len(use_dim) + shift_height], floor32 or None)"""
    use = list(range(use_dim)) if isinstance(use_dim, int) else list(use_dim)
    pts = np.asarray(raw, np.float32)[:, use]
    if not shift_height:
        return pts, None
    with np.errstate(invalid="ignore"):
        fl = floor_height(pts[:, 2])
        h = pts[:, 2] - fl
    return np.concatenate([pts[:, :3], h[:, None], pts[:, 3:]], 1).astype(np.float32), fl


def normalize_color(points, color_mean=None):
    out = np.array(points, np.float32)
    c = out[:, -3:]
    if color_mean is not None:
        c = c - np.asarray(color_mean, np.float32)
    out[:, -3:] = c / np.float32(255.0)
    return out


def same(a, b):
    """value-equal with equal NaN positions (-0.0 == +0.0)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])
