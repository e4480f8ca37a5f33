"""High-resolution occupancy grids from SDF fields: sign-change detection on sub-sampled voxels
(``code_single/tools/extract_occgrid.py:93-147``) on the lattice the voxels SHARE, classified and compacted on the device
(csrc/misc.hip ``nsim_occgrid_*``).

Semantics (the tool's, restated; tests/occgrid_ref.py restates them once more in numpy / plain torch):
  * ``resolution = ((aabb_world[1] - aabb_world[0]) / occ_res).long()`` truncates, so the voxel edge is extent / resolution;
  * voxel (ix, iy, iz) has (s + 1)^3 sample points at per-axis index ``i + k / s``, k = 0 .. s; ``c = float(i) + sub[k]`` with
    ``sub = arange(s + 1, f32) / s``, ``cn = (c / resolution) * 2 - 1``, ``x_world = cn * radius3d + center`` of the world box,
    ``x_obj = (R^T (x_world - t)) / scale``;
  * index i with k = s and index i + 1 with k = 0 are the same float (s / s is exactly 1, i + 1.0 is exact), so the voxels share a
    lattice of ``resolution[a] * s + 1`` points per axis, lattice index j at ``float(j // s) + sub[j % s]``.  The tool asks
    (s + 1)^3 points per voxel, the lattice about s^3.  The coordinates are generated on the device with every operation
    rounded on its own (no fused multiply-add, IEEE division): bit-identical to the tool's separate tensor operations, which
    matters because the sign of an SDF near zero depends on them;
  * points outside the object box are not queried and count as +inf; ``pos = sdf > 0`` (0, -0 and NaN are not positive); a voxel
    is occupied iff ``0 < sum(pos) < (s + 1)^3`` and no sample is infinite;
  * the result: int32 triples (ix, iy, iz) in ascending order (``torch.nonzero`` on an [X, Y, Z] array), independent of ``slab``
    and ``chunk`` and the same from run to run (counts -> scan -> emission, no atomics).

Lattices are [LX, LY, LZ] tensors with z fastest and are walked in slabs of voxel layers in x, so the emission order is the
final order and nothing is sorted.  Per slab the host reads ONE number, the occupied count that sizes the emission (host-mapped
words, no stream synchronisation); filling a slab through a query reads the number of points inside the box once per piece.
"""
import math
from typing import Callable, Dict, Optional

import numpy as np
import torch

from . import _lib

SLAB_BUDGET_BYTES = 512 << 20
# f32 value + uint8 state per lattice point, and one flag byte per (lattice plane, voxel in y, voxel in z)
_BYTES_PER_POINT = 5
MAX_SUBSAMPLE = 4
_NOTIFY = None


def _check_s(s) -> int:
    s = int(s)
    if not 1 <= s <= MAX_SUBSAMPLE:
        raise ValueError(f"occgrid: subsample_factor must be 1..{MAX_SUBSAMPLE}, got {s}")
    return s


def default_slab(ry: int, rz: int, s: int, budget_bytes: int = SLAB_BUDGET_BYTES) -> int:
    """Voxel layers in x per slab so that the slab's lattice (values, states, flags) fits the budget."""
    per_layer = (_BYTES_PER_POINT * (ry * s + 1) * (rz * s + 1) + ry * rz) * s
    # the kernels index a slab's lattice points and voxels with fewer than 2^31 of either
    cap = ((1 << 31) - 1) // ((ry * s + 1) * (rz * s + 1)) - 1
    return int(max(1, min(budget_bytes // max(per_layer, 1), cap // s)))


def _notify():
    global _NOTIFY
    if _NOTIFY is None:
        _NOTIFY = _lib.HostNotify(1)
    return _NOTIFY or None


def _classify_slab(lat: torch.Tensor, state: Optional[torch.Tensor], nxs: int, ry: int, rz: int, s: int, ix0: int) -> torch.Tensor:
    """occupied voxels of one slab: lat f32 [nxs s + 1, ry s + 1, rz s + 1] (state uint8, same shape, or None) -> int32 [m, 3]"""
    global _NOTIFY
    dev = lat.device
    flags = torch.empty([(nxs * s + 1) * ry * rz], dtype=torch.uint8, device=dev)
    nb = (nxs * ry * rz + 255) // 256
    cnt = torch.empty([nb], dtype=torch.int32, device=dev)
    tot = torch.empty([1], dtype=torch.int32, device=dev)
    _lib.call("nsim_occgrid_flags", _lib.ptr(lat), _lib.ptr(state), nxs, ry, rz, s, _lib.ptr(flags))
    _lib.call("nsim_occgrid_count", _lib.ptr(flags), nxs, ry, rz, s, _lib.ptr(cnt))
    nt = _notify()
    adr, seq = nt.arm(0) if nt is not None else (None, 0)
    _lib.call("nsim_occgrid_scan", _lib.ptr(cnt), nb, _lib.ptr(tot), adr, seq)
    m = nt.wait(0, seq) if nt is not None else None
    if m is None:                       # no host-mapped words, or the wait timed out: a synchronising read of the device copy
        m = int(tot.item())
        if nt is not None and int(nt.view[0, 1]) != seq:
            _NOTIFY = False             # finished and still not visible: this memory is not host-coherent
    out = torch.empty([m, 3], dtype=torch.int32, device=dev)
    if m > 0:
        _lib.call("nsim_occgrid_emit", _lib.ptr(flags), nxs, ry, rz, s, ix0, _lib.ptr(cnt), _lib.ptr(out))
    return out


def _lattice_res(shape, s: int):
    res = []
    for n in shape:
        if n < s + 1 or (n - 1) % s:
            raise ValueError(f"occgrid: a lattice axis has res * s + 1 points (s = {s}), got {tuple(shape)}")
        res.append((n - 1) // s)
    return res


def occupancy_from_lattice(lat: torch.Tensor, s: int, *, slab: Optional[int] = None, state: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The classifier alone: lattice of SDF values -> occupied voxels int32 [M, 3], rows (ix, iy, iz) ascending.

    ``lat``: device tensor [LX, LY, LZ] (z fastest in memory), ``L = res * s + 1`` points per axis; voxel (ix, iy, iz) owns the
    lattice points ``[ix s .. ix s + s] x [iy s .. iy s + s] x [iz s .. iz s + s]``.  ``state`` (uint8, same shape, optional):
    a non-zero entry marks a point without a value (outside the box, or pruned) -- its voxels are empty and ``lat`` is not read
    there.  ``slab``: voxel layers in x per pass (default from ``SLAB_BUDGET_BYTES``); the result does not depend on it.
    Peak memory besides ``lat``: one flag byte per (lattice plane, voxel in y, voxel in z) of a slab + the output."""
    s = _check_s(s)
    _lib.require_device(lat, "lat")
    if lat.dim() != 3:
        raise ValueError("occgrid: lat must be [LX, LY, LZ]")
    lat = lat.detach().to(torch.float32).contiguous()
    rx, ry, rz = _lattice_res(lat.shape, s)
    if state is not None:
        _lib.require_device(state, "state")
        if state.shape != lat.shape or state.dtype != torch.uint8:
            raise ValueError("occgrid: state must be uint8 of lat's shape")
        state = state.contiguous()
    slab = default_slab(ry, rz, s) if slab is None else max(1, int(slab))
    parts = []
    for ix0 in range(0, rx, slab):
        nxs = min(slab, rx - ix0)
        sl = slice(ix0 * s, (ix0 + nxs) * s + 1)
        parts.append(_classify_slab(lat[sl], None if state is None else state[sl], nxs, ry, rz, s, ix0))
    return torch.cat(parts) if len(parts) > 1 else parts[0]


# ------------------------------------------------------------------------------------------------ lattice points
def _as_f32(v, shape, default):
    """v (tensor, array, number; None: default) as a host f32 tensor of ``shape``"""
    t = default if v is None else v
    t = t.detach() if isinstance(t, torch.Tensor) else torch.as_tensor(t)
    return t.to(torch.float32).cpu().expand(shape).contiguous()


def make_frame(aabb_world, occ_res: float, s: int, rotation=None, translation=None, scale=None, obj_aabb=None):
    """-> (``_lib.OccgridFrame``, resolution [3] ints, aabb_world f32 [2,3] on the host).  ``resolution``, ``center`` and
    ``radius3d`` come from the same f32 tensor operations the tool runs (``AABBSpace(aabb=aabb_world)``)."""
    s = _check_s(s)
    a = _as_f32(aabb_world, (2, 3), None)
    resolution = ((a[1] - a[0]) / occ_res).long()
    res = [int(r) for r in resolution.tolist()]
    if min(res) < 1:
        raise ValueError(f"occgrid: occ_res {occ_res} is larger than the box {(a[1] - a[0]).tolist()}")
    if max(res) * s + 1 >= 1 << 24:
        raise ValueError("occgrid: resolution * subsample_factor + 1 must stay below 2^24 (exact f32 lattice indices)")
    center, radius = (a[1] + a[0]) / 2.0, (a[1] - a[0]) / 2.0
    R = _as_f32(rotation, (3, 3), torch.eye(3))
    t = _as_f32(translation, (3,), torch.zeros(3))
    sc = _as_f32(scale, (3,), torch.ones(3))
    f = _lib.OccgridFrame()
    f.s = s
    for i in range(3):
        f.res[i] = res[i]
        f.center[i], f.radius[i] = float(center[i]), float(radius[i])
        f.trans[i], f.scale[i] = float(t[i]), float(sc[i])
        f.obj_min[i], f.obj_max[i] = -math.inf, math.inf
    for i in range(9):
        f.rot[i] = float(R.reshape(-1)[i])
    if obj_aabb is not None:
        b = _as_f32(obj_aabb, (2, 3), None)
        for i in range(3):
            f.obj_min[i], f.obj_max[i] = float(b[0, i]), float(b[1, i])
    return f, res, a


def lattice_points(frame, j0: int, n_planes: int, dev, accel=None):
    """Object-space coordinates and states of the lattice planes j0 .. j0 + n_planes - 1 in x -> (x_obj f32 [n, LY, LZ, 3],
    state uint8 [n, LY, LZ]: 0 inside the object box, 1 outside, 2 pruned by ``accel``'s thresholded grid)."""
    ly, lz = frame.res[1] * frame.s + 1, frame.res[2] * frame.s + 1
    x = torch.empty([n_planes, ly, lz, 3], dtype=torch.float32, device=dev)
    st = torch.empty([n_planes, ly, lz], dtype=torch.uint8, device=dev)
    _lib.call("nsim_occgrid_points", frame, int(j0), int(n_planes), _lib.ptr(accel.occ_bits) if accel is not None else None,
              accel.meta if accel is not None else None, _lib.ptr(x), _lib.ptr(st))
    return x, st


def accel_cells_of(accel, x_obj: torch.Tensor) -> torch.Tensor:
    """Flat index (x fastest) of the cell of ``accel``'s grid that contains each point of x_obj [n,3], as the pruning rule
    computes it: ``floor((x - aabb_min) * scale)`` clamped into the grid."""
    m = accel.meta
    mn = torch.tensor(list(m.aabb_min), dtype=torch.float32, device=x_obj.device)
    sc = torch.tensor(list(m.scale), dtype=torch.float32, device=x_obj.device)
    res = torch.tensor(list(m.res), dtype=torch.long, device=x_obj.device)
    g = torch.floor((x_obj.float() - mn) * sc).long()
    g = torch.minimum(torch.clamp(g, min=0), res - 1)
    return g[:, 0] + res[0] * (g[:, 1] + res[1] * g[:, 2])


def _extract(query, frame, res, dev, chunk: int, slab: Optional[int], accel=None):
    s = frame.s
    rx, ry, rz = res
    ly, lz = ry * s + 1, rz * s + 1
    P = ly * lz
    slab = default_slab(ry, rz, s) if slab is None else max(1, int(slab))
    chunk = max(int(chunk), 1)
    per = max(1, chunk // P)                 # lattice planes per piece
    parts = []
    n_active = 0
    n_out = torch.zeros([], dtype=torch.long, device=dev)
    keep = None                              # the last lattice plane of the previous slab = this one's first
    for ix0 in range(0, rx, slab):
        nxs = min(slab, rx - ix0)
        npl = nxs * s + 1
        lat = torch.empty([npl, ly, lz], dtype=torch.float32, device=dev)
        state = torch.empty([npl, ly, lz], dtype=torch.uint8, device=dev)
        first = 0
        if keep is not None:
            lat[0].copy_(keep[0])
            state[0].copy_(keep[1])
            first = 1
        for p0 in range(first, npl, per):
            n = min(per, npl - p0)
            x, st = lattice_points(frame, ix0 * s + p0, n, dev, accel)
            state[p0:p0 + n].copy_(st)
            x = x.view(-1, 3)
            stf = st.view(-1)
            n_out += (stf == 1).sum()
            idx = (stf == 0).nonzero()[:, 0]           # (one size read per piece)
            na = int(idx.shape[0])
            n_active += na
            piece = lat[p0:p0 + n].view(-1)
            if na == 0:
                continue
            if na == x.shape[0]:
                for c0 in range(0, na, chunk):
                    piece[c0:c0 + chunk] = query(x[c0:c0 + chunk])
                continue
            xa = torch.empty([na, 3], dtype=torch.float32, device=dev)
            _lib.call("nsim_rows_gather", _lib.ptr(x), _lib.ptr(idx), na, 3, x.shape[0], 0, _lib.ptr(xa))
            vals = torch.empty([na], dtype=torch.float32, device=dev)
            for c0 in range(0, na, chunk):
                vals[c0:c0 + chunk] = query(xa[c0:c0 + chunk])
            piece.zero_()                              # 0 + v = v: the scatter-add writes the queried values
            _lib.call("nsim_rows_scatter_add", _lib.ptr(vals), _lib.ptr(idx), na, 1, piece.shape[0], _lib.ptr(piece))
        parts.append(_classify_slab(lat, state, nxs, ry, rz, s, ix0))
        keep = (lat[-1], state[-1])
    occ = torch.cat(parts) if len(parts) > 1 else parts[0]
    n_lat, n_out = (rx * s + 1) * P, int(n_out.item())
    stats = dict(n_lattice=n_lat, n_queried=n_active, n_out_of_box=n_out, n_pruned=n_lat - n_active - n_out)
    return occ, stats


def _result(occ, res, a, occ_res, stats):
    return dict(occ_corners=occ, resolution=list(res), coord_min=a[0].numpy().copy(), occ_res=float(occ_res), stats=stats)


def extract_occupancy(query_sdf_fn: Callable, *, aabb_world, occ_res: float, subsample_factor: int = 2, rotation=None,
                      translation=None, scale=None, obj_aabb=None, chunk: int = 1 << 22, slab: Optional[int] = None,
                      device=None) -> Dict:
    """Occupied voxels of the world box ``aabb_world`` [2,3] at edge ``occ_res`` for any SDF ``query_sdf_fn(x_obj [n,3]) -> [n]``
    in object coordinates, ``x_obj = (R^T (x_world - translation)) / scale`` (``rotation`` [3,3] object -> world, ``scale`` a
    number or per axis; defaults: identity).  Points outside ``obj_aabb`` [2,3] (default: none) are not queried and empty every
    voxel they belong to.  -> dict(occ_corners int32 [M,3] on the device, resolution [3], coord_min f32 [3] = aabb_world[0],
    occ_res, stats{n_lattice, n_queried, n_out_of_box, n_pruned}).  The module docstring states the semantics.

    The callable is asked in pieces of at most ``chunk`` points.  Peak memory: 5 bytes per lattice point of a slab of ``slab``
    voxel layers in x (default from ``SLAB_BUDGET_BYTES``) + 13 bytes per point of a piece + what the callable needs."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    frame, res, a = make_frame(aabb_world, occ_res, subsample_factor, rotation, translation, scale, obj_aabb)

    def query(x):
        return query_sdf_fn(x).detach().reshape(-1).float()
    with torch.no_grad():
        occ, stats = _extract(query, frame, res, dev, chunk, slab)
    return _result(occ, res, a, occ_res, stats)


def _box_corners(dev) -> torch.Tensor:
    """the 8 corners of [-1, 1]^3"""
    v = torch.tensor([-1.0, 1.0], device=dev)
    return torch.stack(torch.meshgrid(v, v, v, indexing="ij"), dim=-1).view(8, 3)


def model_world_aabb(model, rotation=None, translation=None, scale=None) -> torch.Tensor:
    """The axis-aligned box of the model's object box carried to the world, as the tool derives it (:94-99): the 8 corners of
    ``model.space.aabb``, times ``scale``, rotated and translated; their per-axis min and max -> [2,3] on the model's device."""
    sp = model.space
    dev = sp.aabb.device
    box = sp.unnormalize_coords(_box_corners(dev))
    sc = _as_f32(scale, (3,), torch.ones(3)).to(dev)
    R = _as_f32(rotation, (3, 3), torch.eye(3)).to(dev)
    t = _as_f32(translation, (3,), torch.zeros(3)).to(dev)
    w = (R * (box * sc).unsqueeze(-2)).sum(-1) + t
    return torch.stack([w.min(dim=0).values, w.max(dim=0).values], dim=0)


def extract_occupancy_from_model(model, *, occ_res: float, subsample_factor: int = 2, rotation=None, translation=None,
                                 scale=None, prune: str = "none", slab: Optional[int] = None, chunk: int = 1 << 22) -> Dict:
    """``extract_occupancy`` of a NeuS model's SDF over the world box of ``model.space.aabb`` (``model_world_aabb``), queried
    through the model's no-grad split-precision query on the packed shadow weights (``_sdf_query``), same return value.

    ``prune="accel"`` (opt-in; ``"none"`` is exactly the tool's result) skips the queries in space the model's own occupancy
    grid knows is empty: a lattice point inside the box is *active* iff the cell of ``model.accel``'s thresholded grid that
    contains it, or any of that cell's 26 neighbours (clamped at the border), is occupied.  Inactive points are not queried, and
    a voxel is classified only if none of its (s + 1)^3 points is inactive -- otherwise it is reported empty.  A pruned point is
    never given a sign (the occupancy value is low deep inside solids too: a sentinel "positive" would invent surfaces at the
    inner side of the occupied shell), so the pruned result is by construction a SUBSET of the unpruned one.  The caveat: a
    surface the occupancy grid has lost is lost here too.  ``stats["n_queried"]`` reports how many points were queried."""
    if prune not in ("none", "accel"):
        raise ValueError(f"occgrid: prune must be 'none' or 'accel', got {prune!r}")
    accel = None
    if prune == "accel":
        accel = getattr(model, "accel", None)
        if accel is None or not hasattr(accel, "occ_bits"):
            raise ValueError("occgrid: prune='accel' needs a model with an occupancy grid (model.accel)")
    dev = model.device
    with torch.no_grad():
        aabb_world = model_world_aabb(model, rotation, translation, scale)
        frame, res, a = make_frame(aabb_world, occ_res, subsample_factor, rotation, translation, scale, model.space.aabb)
        grid16, wpack = model._shadow()

        def query(x):
            x = x.contiguous()
            return model._sdf_query(grid16, wpack, x, None, None, None, None, x.shape[0], dev)
        occ, stats = _extract(query, frame, res, dev, chunk, slab, accel)
    return _result(occ, res, a, occ_res, stats)


def write_occgrid_npz(path, result: Dict, *, coord_offset=None, meta: Optional[dict] = None):
    """The tool's file (:154-158): ``occ_corners`` int16 [M,3], ``sidelength`` (the resolution), ``occ_res``, ``coord_min``,
    ``coord_offset``, ``meta``; load with ``np.load(path, allow_pickle=True)``.  Raises ``ValueError`` when a resolution
    exceeds 32767: int16 corners would wrap (the tool wraps silently)."""
    res = [int(r) for r in result["resolution"]]
    if max(res) > 32767:
        raise ValueError(f"occgrid: resolution {res} does not fit the file's int16 corners (at most 32767 per axis)")
    occ = result["occ_corners"]
    occ = occ.cpu().numpy() if isinstance(occ, torch.Tensor) else np.asarray(occ)
    np.savez_compressed(path, occ_corners=occ.astype(np.int16), sidelength=res, occ_res=result["occ_res"],
                        coord_min=np.asarray(result["coord_min"], dtype=np.float32),
                        coord_offset=np.zeros(3) if coord_offset is None else np.asarray(coord_offset), meta=meta or {})
