"""Nearest-neighbour search and chamfer distance (csrc/misc.hip ``nsim_nn_*``, neuralsim_amd/pointcloud.py) against the numpy
restatement tests/pointcloud_ref.py (bit for bit), against an independent float64 k-d tree, on ties, degenerate clouds and
non-finite input, and the LiDAR metrics against the formulas of ``code_single/tools/eval_lidar.py:417-458``."""
import numpy as np
import pytest
import torch

import pointcloud_ref as R

# relative bound of test 2: subtraction, square and two additions of non-negative terms give at most 4 roundings on d2, the
# square root halves that and adds one
KD_REL = 3.0 * 2.0 ** -24
KD_ABS = 1e-30


def _nn(x, y, dev, method, **kw):
    from neuralsim_amd import pointcloud
    stats = {}
    d2, idx = pointcloud.nearest_neighbors(torch.as_tensor(x).to(dev), torch.as_tensor(y).to(dev), method=method, stats=stats, **kw)
    assert d2.dtype == torch.float32 and idx.dtype == torch.int64
    return d2, idx, stats


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_exact(x, y, dev, ref=None, **kw):
    """both methods equal the restatement bit for bit, each other, and themselves on a second run -> (d2, idx, grid stats)"""
    rd, ri = ref if ref is not None else R.nearest_neighbors(x, y)
    out = {}
    for method in ("brute", "grid"):
        d2, idx, st = _nn(x, y, dev, method, **kw)
        print(f"{method}: N={len(x)} M={len(y)} leftover={int(st['leftover'])} "
              f"d2 mismatches={int((_bits(d2.cpu().numpy()) != _bits(rd)).sum())} idx mismatches={int((idx.cpu().numpy() != ri).sum())}")
        assert (_bits(d2.cpu().numpy()) == _bits(rd)).all(), method
        assert (idx.cpu().numpy() == ri).all(), method
        d2b, idxb, _ = _nn(x, y, dev, method, **kw)
        assert torch.equal(d2, d2b) and torch.equal(idx, idxb), f"{method}: two runs differ"
        out[method] = (d2, idx, st)
    assert torch.equal(out["brute"][0], out["grid"][0]) and torch.equal(out["brute"][1], out["grid"][1])
    return out["grid"]


def _assert_kdtree(x, y, d2, idx):
    spatial = pytest.importorskip("scipy.spatial")
    x64, y64 = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    dd, ii = spatial.cKDTree(y64).query(x64)
    d = np.sqrt(d2.cpu().numpy().astype(np.float64))
    idx = idx.cpu().numpy()
    err = np.abs(d - dd)
    tol = KD_REL * dd + KD_ABS
    print(f"k-d tree: max relative distance error {np.max(err / np.maximum(dd, 1e-300)):.3e} (bound {KD_REL:.3e}), "
          f"{int((idx != ii).sum())} indices differ of {len(ii)}")
    assert (err <= tol).all()
    mm = idx != ii
    if mm.any():       # a tie or near-tie: the point returned is as close as the tree's, to the same bound
        alt = np.linalg.norm(x64[mm] - y64[idx[mm]], axis=1)
        assert (np.abs(alt - dd[mm]) <= KD_REL * dd[mm] + KD_ABS).all()


# ------------------------------------------------------------------------------------------------ 1, 2: parity
CLOUDS = {
    "lidar": lambda: (R.lidar_cloud(3000, 1), R.lidar_cloud(5000, 2)),
    "lidar_odd": lambda: (R.lidar_cloud(1237, 3), R.lidar_cloud(1025, 4)),
    "lidar_big": lambda: (R.lidar_cloud(5000, 5), R.lidar_cloud(8000, 6)),
    "cube": lambda: (R.cube_cloud(2049, 1), R.cube_cloud(4099, 2)),
    "cube_small_y": lambda: (R.cube_cloud(777, 3), R.cube_cloud(63, 4)),
    "one_query": lambda: (R.lidar_cloud(1, 7), R.lidar_cloud(3001, 8)),
    "one_point": lambda: (R.lidar_cloud(3001, 9), R.lidar_cloud(1, 10)),
    "few_queries_many_points": lambda: (R.lidar_cloud(100, 11), R.lidar_cloud(9000, 12)),   # splits y over workgroups
}


@pytest.mark.parametrize("name", list(CLOUDS))
def test_nn_equals_restatement_bit_for_bit(backend, name):
    x, y = CLOUDS[name]()
    _assert_exact(x, y, backend)


@pytest.mark.parametrize("name", ["lidar", "cube"])
def test_nn_against_float64_kdtree(backend, name):
    x, y = CLOUDS[name]()
    for method in ("brute", "grid"):
        d2, idx, _ = _nn(x, y, backend, method)
        _assert_kdtree(x, y, d2, idx)


# ------------------------------------------------------------------------------------------------ 3: ties
def test_nn_duplicates_lowest_index_wins(backend):
    y = R.lidar_cloud(2000, 1)
    y[1500:1600] = y[100:200]            # exact duplicates, the earlier copy must win
    y[700] = y[1999]
    x = np.concatenate([y[100:200], y[1990:], R.lidar_cloud(300, 2)])
    d2, idx, _ = _assert_exact(x, y, backend)
    idx = idx.cpu().numpy()
    assert (idx[:100] == np.arange(100, 200)).all() and idx[109] == 700
    assert (d2.cpu().numpy()[:110] == 0).all()


def test_nn_lattice_cell_centres(backend):
    g = np.arange(8, dtype=np.float32)
    y = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    y = y[np.random.default_rng(0).permutation(len(y))]           # index order unrelated to position
    c = np.arange(7, dtype=np.float32) + 0.5
    x = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)     # 8 equidistant neighbours each
    d2, idx, _ = _assert_exact(x, y, backend)
    assert (d2.cpu().numpy() == 0.75).all()
    for occ in (0.5, 16.0):              # other cell sizes, same answer
        _assert_exact(x, y, backend, target_occ=occ)


# ------------------------------------------------------------------------------------------------ 4: leftovers
def test_nn_outliers_use_the_leftover_pass(backend):
    x = R.with_outliers(R.lidar_cloud(3000, 1), 0.01, 5, scale=400.0)
    y = R.with_outliers(R.lidar_cloud(4000, 2), 0.01, 6, scale=400.0)
    _, _, st = _assert_exact(x, y, backend)
    assert int(st["leftover"]) > 0
    # queries only: y's box stays tight, the far queries cannot be settled by the rings
    _, _, st = _assert_exact(x, R.lidar_cloud(4000, 2), backend)
    assert int(st["leftover"]) > 0
    # every ring cap gives the same answer; with none at all every query of a multi-cell grid that is not settled by its own
    # cell goes through the exhaustive pass
    for rings in (0, 1, 9):
        _assert_exact(x, y, backend, max_rings=rings)


def test_nn_far_outliers_in_y_take_the_exhaustive_pass(backend):
    """a few points kilometres away blow up y's box; the cells then hold the whole sweep and every finite query is handed to the
    tiled exhaustive pass (the coarse-grid guard) -- same bits"""
    x = R.lidar_cloud(1500, 1)
    x[3] = np.nan
    y = R.lidar_cloud(4000, 2)
    y[[5, 77, 3000]] = [[5000.0, -50, 2], [100, 9000.0, 2], [-7000.0, -8000.0, 300.0]]
    _, _, st = _assert_exact(x, y, backend, max_cells=4096)
    assert int(st["leftover"]) == 1499


def test_nn_dense_cube_needs_no_leftover_pass(backend):
    c = R.cube_cloud(6000, 1)
    _, _, st = _assert_exact(c[:2500], c[2500:], backend)
    assert int(st["leftover"]) == 0


# ------------------------------------------------------------------------------------------------ 5: outside, degenerate
def test_nn_queries_outside_the_box(backend):
    y = R.lidar_cloud(3000, 1)
    lo, hi = y.min(0), y.max(0)
    mid = (lo + hi) / 2
    xs = []
    for a in range(3):
        for s, far in ((-1, 1.0), (1, 1.0), (-1, 500.0), (1, 500.0), (-1, 1e6), (1, 3e7)):
            p = np.tile(mid, (16, 1)) + np.random.default_rng(a).uniform(-5, 5, (16, 3))
            p[:, a] = (lo[a] - far) if s < 0 else (hi[a] + far)
            xs.append(p)
    xs.append(np.array([[lo[0] - 100, lo[1] - 100, lo[2] - 100], [hi[0] + 100, hi[1] + 100, hi[2] + 100],
                        [1e30, 0, 0], [-3e38, 3e38, 3e38]]))
    x = np.concatenate(xs).astype(np.float32)
    _assert_exact(x, y, backend)


def test_nn_flat_and_degenerate_clouds(backend):
    r = np.random.default_rng(0)
    plane = R.cube_cloud(3000, 1)
    plane[:, 2] = 0.25                                   # zero extent in z
    line = np.zeros((2000, 3), np.float32)
    line[:, 1] = r.uniform(-50, 50, 2000).astype(np.float32)
    line[:, 0], line[:, 2] = 7.0, -3.0
    same = np.tile(np.array([[100.0, -50.0, 2.0]], np.float32), (500, 1))
    x = np.concatenate([R.cube_cloud(600, 2), plane[:100], line[:50], same[:3]])
    for y in (plane, line, same):
        _assert_exact(x, y, backend)
    # x is y: every distance 0, the lowest index of an equal point
    y = R.lidar_cloud(2500, 3)
    y[2000:2100] = y[50:150]
    d2, idx, _ = _assert_exact(y, y, backend)
    want = np.arange(2500)
    want[2000:2100] = np.arange(50, 150)
    assert (d2.cpu().numpy() == 0).all() and (idx.cpu().numpy() == want).all()


# ------------------------------------------------------------------------------------------------ 6: non-finite, empty
def test_nn_non_finite_and_empty(backend):
    from neuralsim_amd import pointcloud
    x = R.lidar_cloud(700, 1)
    y = R.lidar_cloud(1500, 2)
    bad_rows = np.array([0, 3, 64, 700, 1499])
    y[bad_rows] = [[np.nan, 0, 0], [100, np.inf, 2], [100, -50, -np.inf], [np.nan, np.nan, np.nan], [np.inf, np.inf, 0]]
    y[5] = x[5]
    x[7] = [np.nan, 1, 2]
    x[9] = [100, np.inf, 2]
    d2, idx, _ = _assert_exact(x, y, backend)
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    assert not np.isin(idx, bad_rows).any()
    assert np.isinf(d2[[7, 9]]).all() and (idx[[7, 9]] == -1).all()
    assert np.isfinite(np.delete(d2, [7, 9])).all() and not np.isnan(d2).any()
    # y without a single finite point
    allbad = np.full((300, 3), np.nan, np.float32)
    d2, idx, _ = _assert_exact(x, allbad, backend)
    assert np.isinf(d2.cpu().numpy()).all() and (idx.cpu().numpy() == -1).all()
    for method in ("brute", "grid", "auto"):
        d2, idx, _ = _nn(x, np.zeros((0, 3), np.float32), backend, method)
        assert d2.shape == (700,) and torch.isinf(d2).all() and (d2 > 0).all() and (idx == -1).all()
        d2, idx, _ = _nn(np.zeros((0, 3), np.float32), y, backend, method)
        assert d2.shape == (0,) and idx.shape == (0,)
        a, b = pointcloud.chamfer_distance(torch.zeros([0, 3], device=backend), torch.as_tensor(y).to(backend), method=method)
        assert a.shape == (0,) and b.shape == (1500,) and torch.isinf(b).all()


def test_nn_refuses_cpu_tensors_and_bad_shapes():
    from neuralsim_amd import pointcloud
    with pytest.raises(RuntimeError, match="HIP device"):
        pointcloud.nearest_neighbors(torch.zeros([4, 3]), torch.zeros([4, 3]))
    with pytest.raises(ValueError):
        pointcloud.nearest_neighbors(torch.zeros([4, 2]), torch.zeros([4, 3]))


# ------------------------------------------------------------------------------------------------ 7: chamfer, metrics
def test_chamfer_distance(backend):
    from neuralsim_amd import pointcloud
    x = torch.as_tensor(R.lidar_cloud(1200, 1)).to(backend)
    y = torch.as_tensor(R.lidar_cloud(1700, 2)).to(backend)
    dx, _ = pointcloud.nearest_neighbors(x, y)
    dy, _ = pointcloud.nearest_neighbors(y, x)
    sx, sy = pointcloud.chamfer_distance(x, y, squared=True)
    assert torch.equal(sx, dx) and torch.equal(sy, dy)
    cx, cy = pointcloud.chamfer_distance(x, y)
    assert cx.shape == (1200,) and cy.shape == (1700,)
    assert torch.equal(cx, dx.sqrt()) and torch.equal(cy, dy.sqrt())
    # the square of the default is squared=True up to one rounding of the root (relative 2^-24, doubled by the square) and
    # one of the product
    for c, s in ((cx, sx), (cy, sy)):
        assert ((c * c - s).abs() <= 3 * 2.0 ** -24 * s).all()
    for method in ("brute", "grid"):
        mx, my = pointcloud.chamfer_distance(x, y, method=method)
        assert torch.equal(mx, cx) and torch.equal(my, cy)
    xb = torch.stack([x[:1000], x[200:1200]])
    yb = torch.stack([y[:1500], y[100:1600]])
    bx, by = pointcloud.chamfer_distance(xb, yb)
    assert bx.shape == (2, 1000) and by.shape == (2, 1500)
    for b in range(2):
        lx, ly = pointcloud.chamfer_distance(xb[b], yb[b])
        assert torch.equal(bx[b], lx) and torch.equal(by[b], ly)


def test_lidar_metrics_reproduce_the_tool_formulas(backend):
    """eval_lidar.py:417-458 restated with torch on the same distances"""
    from neuralsim_amd import pointcloud
    gt = R.lidar_cloud(2100, 1)
    origin = np.array([100.0, -50.0, 2.0], np.float32)
    rng = np.random.default_rng(3)
    gt_ranges = np.linalg.norm(gt - origin, axis=1).astype(np.float32)
    pred_ranges = (gt_ranges * (1 + 0.02 * rng.standard_normal(2100)) + 0.05 * rng.standard_normal(2100)).astype(np.float32)
    pred = (origin + (gt - origin) / gt_ranges[:, None] * pred_ranges[:, None]).astype(np.float32)
    keep = rng.random(2100) > 0.1                       # the rays the rendered mask kept
    pred, pred_ranges, gt_ranges_of_pred = pred[keep], pred_ranges[keep], gt_ranges[keep]
    t = lambda a: torch.as_tensor(a).to(backend)
    m = pointcloud.lidar_metrics(t(pred), t(gt), t(pred_ranges), t(gt_ranges_of_pred))

    cham_pred, cham_gt = pointcloud.chamfer_distance(t(pred), t(gt))
    cham_pred_sorted = torch.sort(cham_pred).values
    cham_gt_sorted = torch.sort(cham_gt).values
    err = (t(pred_ranges) - t(gt_ranges_of_pred)).abs()
    err_sorted = torch.sort(err)[0]
    want = {"chamfer_pred": cham_pred.mean().item(), "chamfer_gt": cham_gt.mean().item(),
            "depth_rmse": err.square().mean().sqrt().item()}
    for tag, f in (("99", 0.99), ("97", 0.97), ("95", 0.95)):
        want[f"chamfer_pred_{tag}"] = cham_pred_sorted[0:int(cham_pred_sorted.numel() * f)].mean().item()
        want[f"chamfer_gt_{tag}"] = cham_gt_sorted[0:int(cham_gt_sorted.numel() * f)].mean().item()
        want[f"depth_rmse_{tag}"] = err_sorted[0:int(err_sorted.numel() * f)].square().mean().sqrt().item()
    want["chamfer"] = want["chamfer_pred"] + want["chamfer_gt"]
    for tag in ("99", "97", "95"):
        want[f"chamfer_{tag}"] = want[f"chamfer_pred_{tag}"] + want[f"chamfer_gt_{tag}"]
    assert set(m) == set(want)
    for k, v in want.items():
        assert m[k] == v, k
    assert m["chamfer_95"] <= m["chamfer_97"] <= m["chamfer_99"] <= m["chamfer"]
    assert m["depth_rmse_95"] <= m["depth_rmse_97"] <= m["depth_rmse_99"] <= m["depth_rmse"]
    assert 0 < m["chamfer_pred"] < 5 and 0 < m["depth_rmse"] < 5


# ------------------------------------------------------------------------------------------------ 8: shim
def test_shim_exports_chamfer_distance(backend):
    from nr3d_lib.maths import chamfer_distance
    from neuralsim_amd import pointcloud
    assert chamfer_distance is pointcloud.chamfer_distance
    x = torch.as_tensor(R.cube_cloud(300, 1)).to(backend)
    y = torch.as_tensor(R.cube_cloud(400, 2)).to(backend)
    a, b = chamfer_distance(x, y)                       # the call of eval_lidar.py:419-421: two [N, 3] tensors, positional
    assert a.shape == (300,) and b.shape == (400,)


# ------------------------------------------------------------------------------------------------ 10: full size
@pytest.mark.gpu
def test_nn_full_sweep_on_the_gpu():
    """2 x 10^5 against 2 x 10^5 LiDAR-like points: grid equals brute exactly, both directions, and the float64 tree"""
    assert torch.cuda.is_available()
    dev = torch.device("cuda", 0)
    x, y = R.lidar_cloud(200000, 21), R.lidar_cloud(200000, 22)
    y[150000:150050] = y[10:60]
    for a, b in ((x, y), (y, x)):
        bd, bi, _ = _nn(a, b, dev, "brute")
        gd, gi, st = _nn(a, b, dev, "grid")
        print(f"full sweep: leftover {int(st['leftover'])} of {len(a)}")
        assert torch.equal(bd, gd) and torch.equal(bi, gi)
        gd2, gi2, _ = _nn(a, b, dev, "grid")
        assert torch.equal(gd, gd2) and torch.equal(gi, gi2)
        _assert_kdtree(a, b, gd, gi)
