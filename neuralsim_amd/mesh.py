"""Mesh extraction from SDF fields: marching cubes on the device (csrc/misc.hip ``nsim_mc_*``) and a binary PLY writer.

``nr3d_lib.graphics.trianglemesh.extract_mesh`` is called by ``code_single/tools/extract_mesh.py:124`` and
``code_multi/tools/extract_mesh.py:73``; the library itself is not vendored, so its conventions are restated here
(``extract_mesh``'s docstring).  ``extract_mesh_from_model`` is the fast path without Python callables: lattice points are
generated on the device and fed to the model's no-grad split-precision query (``_sdf_query``, the occupancy refresh's path).

The marching-cubes conventions (table, orientation, vertex and triangle order, non-finite corners) are stated in
csrc/misc.hip; tests/mesh_ref.py restates them in numpy.
"""
import math
import sys
from typing import Callable, Dict, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib

# default lattice budget of one slab: f32 values + three int32 vertex-id planes = 16 bytes per lattice point
SLAB_BUDGET_BYTES = 512 << 20
_BYTES_PER_POINT = 16
_ID_LIMIT = (1 << 31) - 1


def default_slab(nx: int, ny: int, budget_bytes: int = SLAB_BUDGET_BYTES) -> int:
    """Cubes per slab in z so that a slab's lattice (its planes + the two neighbour planes) and vertex ids fit the budget."""
    per_plane = _BYTES_PER_POINT * int(nx) * int(ny)
    return int(max(1, min(65534, budget_bytes // max(per_plane, 1) - 3)))


def _planes_of(src, k0: int, n: int, ny: int, nx: int, dev):
    """planes [k0, k0 + n) of a lattice tensor, or filled by the callable ``src(k0, n, out)``"""
    if isinstance(src, torch.Tensor):
        return src[k0:k0 + n]
    out = torch.empty([n, ny, nx], dtype=torch.float32, device=dev)
    src(k0, n, out)
    return out


def marching_cubes(lattice: Union[torch.Tensor, Callable], bmin: Sequence[float], h: float, level: float = 0.0, *,
                   shape: Optional[Sequence[int]] = None, slab: Optional[int] = None,
                   budget_bytes: int = SLAB_BUDGET_BYTES, device=None):
    """The surface {value = level} of a lattice of values -> (verts [V,3] f32, faces [F,3] int32, normals [V,3] f32), all on
    the device.

    ``lattice``: a device tensor f32 [nz, ny, nx] (x fastest), or a callable ``fill(k0, n, out)`` that writes lattice planes
    k0 .. k0 + n - 1 into the device tensor ``out`` [n, ny, nx]; the callable needs ``shape = (nx, ny, nz)`` and ``device``.
    Lattice point (i, j, k) sits at ``bmin + h (i, j, k)``.  The grid is walked in z-slabs of ``slab`` cubes (default: from
    ``budget_bytes``); a callable is asked for every plane once, plus the planes next to a slab border for the normals,
    so the peak memory is bounded by the slab, not by the grid."""
    if isinstance(lattice, torch.Tensor):
        _lib.require_device(lattice, "lattice")
        if lattice.dim() != 3:
            raise ValueError("marching_cubes: lattice must be [nz, ny, nx]")
        lattice = lattice.detach().to(torch.float32).contiguous()
        nz, ny, nx = (int(s) for s in lattice.shape)
        dev = lattice.device
    else:
        if shape is None or device is None:
            raise ValueError("marching_cubes: a lattice callable needs shape=(nx, ny, nz) and device")
        nx, ny, nz = (int(s) for s in shape)
        dev = torch.device(device)
    bx, by, bz = (float(v) for v in bmin)
    h = float(h)
    empty = (torch.zeros([0, 3], dtype=torch.float32, device=dev), torch.zeros([0, 3], dtype=torch.int32, device=dev),
             torch.zeros([0, 3], dtype=torch.float32, device=dev))
    if nx < 1 or ny < 1 or nz < 1:
        return empty
    slab = default_slab(nx, ny, budget_bytes) if slab is None else int(slab)
    slab = max(1, min(slab, 65534))
    P = nx * ny
    bpp = (P + 255) // 256
    verts, faces, normals = [], [], []
    vbase = 0
    prev = None          # (global index of the first plane held, planes [m, ny, nx]) -- a callable's planes kept for the next slab
    k0 = 0
    while True:
        nzs = min(slab, nz - 1 - k0)
        k1 = k0 + nzs
        last = k1 == nz - 1
        lo, hi = max(k0 - 1, 0), min(k1 + 1, nz - 1)
        if isinstance(lattice, torch.Tensor):
            win = lattice[lo:hi + 1]
        else:
            have = 0
            parts = []
            if prev is not None:          # the planes of the previous window that this one needs again
                p0, pw = prev
                a = lo - p0
                if 0 <= a < pw.shape[0]:
                    parts.append(pw[a:])
                    have = pw.shape[0] - a
            need = hi + 1 - (lo + have)
            if need > 0:
                parts.append(_planes_of(lattice, lo + have, need, ny, nx, dev))
            win = parts[0] if len(parts) == 1 else torch.cat(parts)
            prev = (lo, win)
        win = win.contiguous()
        body = win[k0 - lo:k0 - lo + nzs + 1]
        below = win[0] if k0 > 0 else None
        above = win[-1] if not last else None
        cnt_v = torch.empty([(nzs + 1) * 2 * bpp], dtype=torch.int32, device=dev)
        cnt_t = torch.empty([(nzs + 1) * bpp], dtype=torch.int32, device=dev)
        tot = torch.zeros([3], dtype=torch.int32, device=dev)
        _lib.call("nsim_mc_count", _lib.ptr(body), nx, ny, nzs, float(level), _lib.ptr(cnt_v), _lib.ptr(cnt_t))
        _lib.call("nsim_mc_scan", _lib.ptr(cnt_v), _lib.ptr(cnt_t), nx, ny, nzs, _lib.ptr(tot))
        n_before_top, n_all, n_tri = (int(v) for v in tot.cpu().tolist())
        n_emit = n_all if last else n_before_top
        if vbase + n_all > _ID_LIMIT:
            raise RuntimeError("marching_cubes: more than 2^31 - 1 vertices (int32 face indices)")
        vid = torch.empty([3, nzs + 1, P], dtype=torch.int32, device=dev)
        v = torch.empty([max(n_emit, 1), 3], dtype=torch.float32, device=dev)
        n = torch.empty([max(n_emit, 1), 3], dtype=torch.float32, device=dev)
        _lib.call("nsim_mc_emit_verts", _lib.ptr(body), _lib.ptr(below.contiguous() if below is not None else None),
                  _lib.ptr(above.contiguous() if above is not None else None), nx, ny, nzs, float(level), bx, by, bz, h,
                  k0, vbase, 1 if last else 0, _lib.ptr(cnt_v), _lib.ptr(vid), _lib.ptr(v), _lib.ptr(n))
        f = torch.empty([max(n_tri, 1), 3], dtype=torch.int32, device=dev)
        if n_tri > 0:
            _lib.call("nsim_mc_emit_tris", _lib.ptr(body), nx, ny, nzs, float(level), _lib.ptr(cnt_t), _lib.ptr(vid), _lib.ptr(f))
        verts.append(v[:n_emit])
        normals.append(n[:n_emit])
        faces.append(f[:n_tri])
        vbase += n_emit
        if last:
            break
        k0 = k1
    return torch.cat(verts), torch.cat(faces), torch.cat(normals)


# ------------------------------------------------------------------------------------------------ PLY
def write_ply(filepath: str, verts: np.ndarray, faces: np.ndarray, colors: Optional[np.ndarray] = None):
    """Binary little-endian PLY: ``float x, y, z`` [+ ``uchar red, green, blue``] per vertex, ``list uchar int
    vertex_indices`` per face."""
    verts = np.ascontiguousarray(verts, dtype="<f4").reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype="<i4").reshape(-1, 3)
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {verts.shape[0]}",
            "property float x", "property float y", "property float z"]
    fields = [("xyz", "<f4", (3,))]
    if colors is not None:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
        fields.append(("rgb", "u1", (3,)))
    head += [f"element face {faces.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    vrec = np.empty(verts.shape[0], dtype=fields)
    vrec["xyz"] = verts
    if colors is not None:
        vrec["rgb"] = np.ascontiguousarray(colors, dtype=np.uint8).reshape(-1, 3)
    frec = np.empty(faces.shape[0], dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    frec["n"] = 3
    frec["idx"] = faces
    with open(filepath, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


def _postprocess(verts, faces, normals, query_color_fn, include_color, chunk, scale, transform, filepath):
    """colours, scale / transform, PLY: -> dict of host arrays"""
    colors = None
    if include_color:
        if query_color_fn is None:
            raise ValueError("extract_mesh: include_color needs query_color_fn")
        cols = []
        for s in range(0, verts.shape[0], chunk):
            x, v = verts[s:s + chunk], -normals[s:s + chunk]
            cols.append(query_color_fn(x, v).detach().float().reshape(-1, 3))
        c = torch.cat(cols) if cols else verts.new_zeros([0, 3])
        colors = (c.clamp(0.0, 1.0) * 255.0).round().to(torch.uint8).cpu().numpy()
    v = verts.cpu().numpy().astype(np.float64)
    if scale is not None:
        v = v * np.asarray(scale, dtype=np.float64).reshape(-1)[None, :] if np.ndim(scale) else v * float(scale)
    if transform is not None:
        T = np.asarray(transform.cpu() if isinstance(transform, torch.Tensor) else transform, dtype=np.float64).reshape(4, 4)
        v = v @ T[:3, :3].T + T[:3, 3]
    out = dict(verts=v.astype(np.float32), faces=faces.cpu().numpy().astype(np.int32),
               normals=normals.cpu().numpy().astype(np.float32), colors=colors)
    if filepath is not None:
        write_ply(filepath, out["verts"], out["faces"], colors)
    return out


def lattice_shape(bmin, bmax, N: int):
    """(h, (nx, ny, nz)): isotropic spacing h = min(bmax - bmin) / (N - 1), n_a = round(size_a / h) + 1"""
    size = [float(b) - float(a) for a, b in zip(bmin, bmax)]
    h = min(size) / (int(N) - 1)
    return h, tuple(int(round(s / h)) + 1 for s in size)


def _lattice_points(bmin, h: float, nx: int, ny: int, k0: int, n: int, dev) -> torch.Tensor:
    """lattice points of planes [k0, k0 + n): [n, ny, nx, 3] f32, x = bmin + h (i, j, k)"""
    ar = [torch.arange(m, dtype=torch.float32, device=dev) for m in (nx, ny)]
    kk = torch.arange(k0, k0 + n, dtype=torch.float32, device=dev)
    b = torch.tensor([float(v) for v in bmin], dtype=torch.float32, device=dev)
    zz, yy, xx = torch.meshgrid(kk, ar[1], ar[0], indexing="ij")
    return torch.stack([xx, yy, zz], dim=-1) * h + b


def extract_mesh(query_sdf_fn: Callable, query_color_fn: Optional[Callable] = None, *, bmin, bmax, N: int = 512,
                 chunk: int = 16 * 1024, level: float = 0.0, include_color: bool = False, filepath: Optional[str] = None,
                 show_progress: bool = True, scale=None, transform=None, device=None, slab: Optional[int] = None) -> Dict:
    """``nr3d_lib.graphics.trianglemesh.extract_mesh`` (code_single/tools/extract_mesh.py:124, code_multi/tools/extract_mesh.py:73).

    Conventions restated here (the library is not vendored):
      * isotropic spacing ``h = min(bmax - bmin) / (N - 1)``; ``n_a = round(size_a / h) + 1`` lattice points per axis,
        starting at ``bmin``;
      * the lattice points are queried through ``query_sdf_fn(x [n,3]) -> [n]`` in chunks of ``chunk`` points, slab by slab;
      * the surface is {sdf = level}, extracted on the device (``marching_cubes``);
      * colours = ``query_color_fn(verts, -normals)``, clamped to [0, 1] and stored as uchar;
      * ``v' = transform @ [scale * v, 1]``, ``scale`` a float or a per-axis array, ``transform`` a 4x4 matrix;
      * ``filepath``: a binary little-endian PLY (``float x,y,z``, optional ``uchar red,green,blue``,
        ``list uchar int vertex_indices``).
    Returns dict(verts, faces, normals, colors) as host arrays (after scale / transform; normals in the lattice frame).
    ``device`` (default: the current HIP device) holds the lattice; ``slab``: cubes per slab in z (default from a budget)."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    h, (nx, ny, nz) = lattice_shape(bmin, bmax, N)
    chunk = max(int(chunk), 1)
    progress = None
    if show_progress:
        try:
            from tqdm import tqdm
            progress = tqdm(total=nz, desc="extract_mesh", file=sys.stderr)
        except ImportError:
            progress = None

    def fill(k0, n, out):
        x = _lattice_points(bmin, h, nx, ny, k0, n, dev).reshape(-1, 3)
        o = out.view(-1)
        for s in range(0, x.shape[0], chunk):
            o[s:s + chunk] = query_sdf_fn(x[s:s + chunk]).detach().reshape(-1).float()
        if progress is not None:
            progress.update(n)

    with torch.no_grad():
        verts, faces, normals = marching_cubes(fill, bmin, h, level, shape=(nx, ny, nz), slab=slab, device=dev)
        if progress is not None:
            progress.close()
        return _postprocess(verts, faces, normals, query_color_fn, include_color, chunk, scale, transform, filepath)


def model_lattice_fill(model, N: int, chunk: int = 1 << 22):
    """-> (fill(k0, n, out), h, (nx, ny, nz), bmin) over ``model.space.aabb`` with ``extract_mesh``'s lattice conventions;
    the lattice values come from the model's no-grad query (object coordinates) in chunks of ``chunk`` points."""
    a = model.space.aabb.detach().cpu()
    bmin, bmax = a[0].tolist(), a[1].tolist()
    h, shape = lattice_shape(bmin, bmax, N)
    nx, ny, _ = shape
    dev = model.device

    @torch.no_grad()
    def fill(k0, n, out):
        grid16, wpack = model._shadow()
        o = out.view(-1)
        # planes in pieces of at most ``chunk`` points (the level-major planes of the query take 64-128 bytes per point)
        per = max(1, chunk // (nx * ny))
        for k in range(k0, k0 + n, per):
            m = min(per, k0 + n - k)
            x = _lattice_points(bmin, h, nx, ny, k, m, dev).reshape(-1, 3).contiguous()
            s = (k - k0) * nx * ny
            o[s:s + x.shape[0]] = model._sdf_query(grid16, wpack, x, None, None, None, None, x.shape[0], dev)
    return fill, h, shape, bmin


def extract_mesh_from_model(model, N: int, level: float = 0.0, *, include_color: bool = False, h_appear=None,
                            slab: Optional[int] = None, filepath: Optional[str] = None, chunk: int = 1 << 22) -> Dict:
    """Mesh of ``model``'s surface {sdf = level} over its AABB on an N-point lattice (shortest axis): lattice points generated
    on the device, the no-grad query, marching cubes, optionally colours from ``model.forward(verts, -normals, h_appear=)``;
    same conventions and return value as ``extract_mesh``."""
    fill, h, shape, bmin = model_lattice_fill(model, N, chunk)
    with torch.no_grad():
        verts, faces, normals = marching_cubes(fill, bmin, h, level, shape=shape, slab=slab, device=model.device)

        def color_fn(x, v):
            ha = None if h_appear is None else h_appear.reshape(1, -1).expand(x.shape[0], -1).contiguous()
            return model.forward(x, v, with_rgb=True, with_normal=False, h_appear=ha)["rgb"]
        return _postprocess(verts, faces, normals, color_fn, include_color, 1 << 20, None, None, filepath)
