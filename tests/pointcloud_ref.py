"""numpy restatement of the nearest-neighbour search of csrc/misc.hip (``nsim_nn_*``) and the seeded test clouds.

``nearest_neighbors``: for every query the f32 minimum of ``(dx*dx + dy*dy) + dz*dz`` over the points of ``y`` (each operation
rounded to f32, in that order) and numpy's first-occurrence ``argmin``; rows of ``y`` with a non-finite coordinate never win; a
query no point was selected for (non-finite query, empty ``y``) gets ``+inf`` / ``-1``."""
import numpy as np


def nearest_neighbors(x, y, chunk=256):
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 3)
    y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1, 3)
    n, m = len(x), len(y)
    d2 = np.full(n, np.inf, dtype=np.float32)
    idx = np.full(n, -1, dtype=np.int64)
    if n == 0 or m == 0:
        return d2, idx
    bad = ~np.isfinite(y).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, n, chunk):
            d = x[s:s + chunk, None, :] - y[None, :, :]
            q = d * d
            v = (q[..., 0] + q[..., 1]) + q[..., 2]
            assert v.dtype == np.float32
            v[:, bad] = np.inf
            v[np.isnan(v)] = np.inf          # non-finite queries
            a = v.argmin(axis=1)
            mn = v[np.arange(len(a)), a]
            d2[s:s + chunk] = mn
            idx[s:s + chunk] = np.where(np.isinf(mn), -1, a)
    return d2, idx


def lidar_cloud(n, seed, origin=(100.0, -50.0, 2.0)):
    """A LiDAR-like sweep: uniform azimuth, elevation in [-22 deg, +2.5 deg], returns from the ground plane z = -2 and two side
    walls |y| = 12 (sensor frame), range capped at 75 m, sensor at ``origin`` so that world coordinates are large."""
    r = np.random.default_rng(seed)
    az = r.random(n) * 2 * np.pi
    el = np.deg2rad(-22.0 + 24.5 * r.random(n))
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1)
    t_g = np.where(d[:, 2] < 0, -2.0 / np.minimum(d[:, 2], -1e-9), 1e9)
    t_w = 12.0 / np.maximum(np.abs(d[:, 1]), 1e-9)
    t = np.minimum(np.minimum(t_g, t_w), 75.0)
    return (d * t[:, None] + np.asarray(origin)).astype(np.float32)


def cube_cloud(n, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, size=(n, 3)).astype(np.float32)


def with_outliers(c, frac, seed, scale=3000.0):
    """``frac`` of the points thrown far away (up to ``scale`` from the cloud's first point)"""
    r = np.random.default_rng(seed)
    c = c.copy()
    k = max(1, int(len(c) * frac))
    sel = r.choice(len(c), size=k, replace=False)
    c[sel] = c[0] + r.uniform(-scale, scale, size=(k, 3)).astype(np.float32)
    return c
