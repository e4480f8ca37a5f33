"""Point-cloud operators on the device: exact nearest neighbours, chamfer distance, and the LiDAR evaluation metrics.

``nr3d_lib.maths.chamfer_distance`` is called by ``code_single/tools/eval_lidar.py:417-421``; the library itself is not vendored.
The kernels (csrc/misc.hip ``nsim_nn_*``) return, for every query, the squared distance to its nearest point of the other cloud
-- ``(dx*dx + dy*dy) + dz*dz`` in f32 -- and the lowest index that attains it, bit-identical between the exhaustive and the grid
path and from run to run; tests/pointcloud_ref.py restates that in numpy.

Whether nr3d_lib's ``chamfer_distance`` returns distances or squared distances cannot be read anywhere.  Its call site takes
means of the values, reports them next to a range RMSE in metres and colours them with a ceiling of 1.0 next to 5.0 m for the
range error (``eval_lidar.py:119-120``): that fits metres, so ``chamfer_distance`` returns Euclidean distances and
``squared=True`` switches.  This is a reading of the call site, not of the source.
"""
from typing import Dict, Optional, Tuple

import torch

from . import _lib

# Constants of the grid path; the measurements behind them are in profiles/nn_search.md.
GRID_TARGET_OCC = 4.0          # mean points per occupied cell the cell size aims at
GRID_MAX_RINGS = 4             # rings of cells before a query goes to the exhaustive pass
GRID_CELLS_PER_POINT = 4       # the cell budget: this many cells per point of y ...
GRID_MAX_CELLS = 1 << 22       # ... at most this many (one workgroup scans the counts), at least GRID_MIN_CELLS
GRID_MIN_CELLS = 4096
AUTO_BRUTE_PAIRS = 1 << 30     # method="auto": exhaustive search up to this many (query, point) pairs (measured crossover)
_CUS = 256                     # workgroups the exhaustive search wants in flight before it stops splitting y
_SPLIT_BUDGET_BYTES = 128 << 20  # partial results of a split exhaustive search: 8 bytes per (chunk, query)
_HDR_INTS = 32
_HDR_LEFT = 7                  # include/nsim.h: hdr[7] = queries handed to the exhaustive pass


def _cloud(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[-1] != 3:
        raise ValueError(f"{name} must be a [N, 3] tensor, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)}")
    _lib.require_device(t, name)
    return t.detach().to(torch.float32).contiguous()


def _nsplit(n_queries: int, m: int, row: int) -> int:
    """Chunks of y per query block: enough workgroups to fill the device, within the budget of the partial results
    (``row`` = their row length)."""
    qb = (n_queries + 255) // 256
    if qb >= _CUS or m <= 1024:
        return 1
    want = (4 * _CUS + qb - 1) // qb
    return int(max(1, min(want, (m + 1023) // 1024, _SPLIT_BUDGET_BYTES // (8 * max(row, 1)), 65535)))


def _brute(x, y, d2, idx, qlist=None, nq=None, nsplit=1):
    n = x.shape[0]
    part_d2 = part_idx = None
    if nsplit > 1:
        part_d2 = torch.empty([nsplit, n], dtype=torch.float32, device=x.device)
        part_idx = torch.empty([nsplit, n], dtype=torch.int32, device=x.device)
    _lib.call("nsim_nn_brute", _lib.ptr(x), n, _lib.ptr(y), y.shape[0], _lib.ptr(qlist), _lib.ptr(nq), nsplit,
              _lib.ptr(part_d2), _lib.ptr(part_idx), _lib.ptr(d2), _lib.ptr(idx))


def nearest_neighbors(x: torch.Tensor, y: torch.Tensor, *, method: str = "auto", target_occ: Optional[float] = None,
                      max_rings: Optional[int] = None, max_cells: Optional[int] = None,
                      stats: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Nearest point of ``y`` [M, 3] for every point of ``x`` [N, 3] -> (d2 [N] f32 squared distances, idx [N] int64), on the
    current stream of the inputs' device, without a host synchronisation.

    ``d2[i] = min_j ((dx*dx + dy*dy) + dz*dz)`` in f32 and ``idx[i]`` is the lowest ``j`` that attains it.  Points of ``y``
    with a non-finite coordinate are never returned; a query with a non-finite coordinate, or an empty ``y``, gets
    ``d2 = +inf``, ``idx = -1``.  ``method``: ``"brute"`` (tiled exhaustive search), ``"grid"`` (uniform grid over ``y``, the
    queries it cannot settle within ``max_rings`` rings of cells finished exhaustively) or ``"auto"`` (by size); all return
    the same bits.  ``stats`` (a dict) receives ``method`` and, for the grid path, ``leftover``: a device int32 scalar, the
    number of queries that went to the exhaustive pass."""
    if method not in ("auto", "grid", "brute"):
        raise ValueError(f"nearest_neighbors: unknown method {method!r}")
    x = _cloud(x, "x")
    y = _cloud(y, "y")
    if x.device != y.device:
        raise ValueError("nearest_neighbors: x and y must live on the same device")
    dev = x.device
    n, m = int(x.shape[0]), int(y.shape[0])
    if method == "auto":
        method = "brute" if n * m <= AUTO_BRUTE_PAIRS else "grid"
    if stats is not None:
        stats["method"] = method
        stats["leftover"] = torch.zeros([], dtype=torch.int32, device=dev)
    if n == 0:
        return torch.zeros([0], dtype=torch.float32, device=dev), torch.zeros([0], dtype=torch.int64, device=dev)
    if m == 0:
        return (torch.full([n], float("inf"), dtype=torch.float32, device=dev),
                torch.full([n], -1, dtype=torch.int64, device=dev))
    d2 = torch.empty([n], dtype=torch.float32, device=dev)
    idx = torch.empty([n], dtype=torch.int32, device=dev)
    if method == "brute":
        _brute(x, y, d2, idx, nsplit=_nsplit(n, m, n))
        return d2, idx.to(torch.int64)
    occ = GRID_TARGET_OCC if target_occ is None else float(target_occ)
    rings = GRID_MAX_RINGS if max_rings is None else int(max_rings)
    cells = int(max_cells) if max_cells is not None else max(GRID_MIN_CELLS, min(GRID_CELLS_PER_POINT * m, GRID_MAX_CELLS))
    # workspace from the caching allocator: header, cell counts / offsets, cell and rank of every point, records, leftover list
    hdr = torch.empty([_HDR_INTS], dtype=torch.int32, device=dev)
    cell_cnt = torch.empty([cells + 1], dtype=torch.int32, device=dev)
    cell_of = torch.empty([m], dtype=torch.int32, device=dev)
    rank = torch.empty([m], dtype=torch.int32, device=dev)
    rec = torch.empty([m, 4], dtype=torch.float32, device=dev)
    left = torch.empty([n], dtype=torch.int32, device=dev)
    _lib.call("nsim_nn_grid_count", _lib.ptr(y), m, occ, cells, _lib.ptr(hdr), _lib.ptr(cell_cnt), _lib.ptr(cell_of), _lib.ptr(rank))
    _lib.call("nsim_nn_grid_scan", _lib.ptr(hdr), _lib.ptr(cell_cnt))
    _lib.call("nsim_nn_grid_fill", _lib.ptr(y), m, _lib.ptr(cell_cnt), _lib.ptr(cell_of), _lib.ptr(rank), _lib.ptr(rec))
    _lib.call("nsim_nn_grid_query", _lib.ptr(x), n, _lib.ptr(rec), _lib.ptr(cell_cnt), _lib.ptr(hdr), rings, _lib.ptr(d2),
              _lib.ptr(idx), _lib.ptr(left))
    n_left = hdr[_HDR_LEFT:_HDR_LEFT + 1]
    # the host does not know how many queries are left: the launch covers up to 1024 query blocks (the kernel strides over a
    # longer list), the workgroups beyond the list leave at once, and y is split as for a short list (few queries against
    # all of y is the case the split exists for)
    _brute(x, y, d2, idx, qlist=left, nq=n_left, nsplit=_nsplit(1, m, n))
    if stats is not None:
        stats["leftover"] = n_left[0]
        stats["hdr"] = hdr
    return d2, idx.to(torch.int64)


def chamfer_distance(x: torch.Tensor, y: torch.Tensor, *, squared: bool = False, method: str = "auto"):
    """Per-point chamfer terms of two clouds -> (cham_x [N], cham_y [M]): the distance from every point of ``x`` to its nearest
    point of ``y`` and the other way round (``nr3d_lib.maths.chamfer_distance`` as ``eval_lidar.py:417-421`` uses it:
    unbatched ``[N, 3]`` tensors in, two per-point vectors out).  Euclidean distances by default, squared with
    ``squared=True`` (module docstring).  ``[B, N, 3]`` / ``[B, M, 3]`` inputs are looped over and give ``[B, N]``, ``[B, M]``."""
    if x.dim() == 3:
        if y.dim() != 3 or y.shape[0] != x.shape[0]:
            raise ValueError("chamfer_distance: batched x needs y with the same batch size")
        outs = [chamfer_distance(xb, yb, squared=squared, method=method) for xb, yb in zip(x, y)]
        return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])
    dx, _ = nearest_neighbors(x, y, method=method)
    dy, _ = nearest_neighbors(y, x, method=method)
    return (dx, dy) if squared else (dx.sqrt(), dy.sqrt())


def _trimmed(sorted_vals: torch.Tensor, frac: float) -> torch.Tensor:
    return sorted_vals[0:int(sorted_vals.numel() * frac)]


def lidar_metrics(pred_pcl: torch.Tensor, gt_pcl: torch.Tensor, pred_ranges: torch.Tensor, gt_ranges: torch.Tensor) -> Dict[str, float]:
    """The per-frame numbers of ``eval_lidar.py:417-458`` for a rendered sweep ``pred_pcl`` [N, 3] against the measured one
    ``gt_pcl`` [M, 3], and the rendered ranges against the measured ranges of the same beams (both [N]): the mean chamfer terms
    of both directions, their means over the lowest 99 / 97 / 95 % (sorted, cut at ``int(n * frac)``), their sums
    (``chamfer*``), and the RMSE of the absolute range errors, whole and over the same trimmed shares."""
    cham_pred, cham_gt = chamfer_distance(pred_pcl, gt_pcl)
    err = (pred_ranges - gt_ranges).abs()
    cp, cg, es = torch.sort(cham_pred).values, torch.sort(cham_gt).values, torch.sort(err).values
    out = {"chamfer_pred": cham_pred.mean().item(), "chamfer_gt": cham_gt.mean().item(),
           "depth_rmse": err.square().mean().sqrt().item()}
    for tag, frac in (("99", 0.99), ("97", 0.97), ("95", 0.95)):
        out[f"chamfer_pred_{tag}"] = _trimmed(cp, frac).mean().item()
        out[f"chamfer_gt_{tag}"] = _trimmed(cg, frac).mean().item()
        out[f"depth_rmse_{tag}"] = _trimmed(es, frac).square().mean().sqrt().item()
    out["chamfer"] = out["chamfer_pred"] + out["chamfer_gt"]
    for tag in ("99", "97", "95"):
        out[f"chamfer_{tag}"] = out[f"chamfer_pred_{tag}"] + out[f"chamfer_gt_{tag}"]
    return out
