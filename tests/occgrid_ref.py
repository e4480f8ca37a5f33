"""Restatement of ``code_single/tools/extract_occgrid.py:93-147`` for the tests of neuralsim_amd/occgrid.py: the PER-VOXEL
algorithm -- (s + 1)^3 sample points per voxel, nothing shared -- in numpy (a given lattice) and in plain torch with separate
tensor operations (coordinates, a callable SDF in 64^3 blocks).  Test infrastructure; the product never imports it."""
import itertools

import numpy as np
import torch


def classify(lat: np.ndarray, s: int) -> np.ndarray:
    """lat [LX, LY, LZ] (L = res s + 1) -> occupied voxels int [M, 3], ascending (ix, iy, iz): every voxel gathers its own
    (s + 1)^3 values; occupied iff 0 < sum(value > 0) < (s + 1)^3 and no value is infinite."""
    res = [(n - 1) // s for n in lat.shape]
    k = np.arange(s + 1)
    ix = (np.arange(res[0]) * s)[:, None] + k
    iy = (np.arange(res[1]) * s)[:, None] + k
    iz = (np.arange(res[2]) * s)[:, None] + k
    v = lat[ix[:, None, None, :, None, None], iy[None, :, None, None, :, None], iz[None, None, :, None, None, :]]
    v = v.reshape(res[0], res[1], res[2], -1)
    with np.errstate(invalid="ignore"):
        n_pos = (v > 0).sum(-1)
    occ = (n_pos > 0) & (n_pos < (s + 1) ** 3) & ~np.isinf(v).any(-1)
    return np.argwhere(occ)


def resolution_of(aabb_world: torch.Tensor, occ_res: float) -> torch.Tensor:
    return ((aabb_world[1] - aabb_world[0]) / occ_res).long()


def world_to_obj(xw, R, t, scale):
    """``obj.world_transform(x, inv=True) / obj.scale.vec_3()``: broadcast-multiply with the transposed rotation, the three
    products added left to right, then the division"""
    d = xw - t
    p = R.transpose(-1, -2) * d.unsqueeze(-2)
    return ((p[..., 0] + p[..., 1]) + p[..., 2]) / scale


def voxel_coords(block, resolution, s, aabb_world, R, t, scale, dev):
    """sample points of the voxels ``block`` = (index tensors in x, y, z), per voxel: -> x_obj [bx, by, bz, (s + 1)^3, 3]"""
    sub = [torch.arange(s + 1, device=dev, dtype=torch.float) / s for _ in range(3)]
    sub = torch.stack(torch.meshgrid(sub, indexing="ij"), dim=-1).view(-1, 3)
    full = torch.stack(torch.meshgrid(list(block), indexing="ij"), dim=-1)
    coords = full.float().unsqueeze(-2) + sub[None, None, None, :, :]
    center, radius = (aabb_world[1] + aabb_world[0]) / 2.0, (aabb_world[1] - aabb_world[0]) / 2.0
    xw = ((coords / resolution) * 2 - 1) * radius + center
    return world_to_obj(xw, R, t, scale)


def extract_per_voxel(query, *, aabb_world, occ_res, s, R, t, scale, obj_aabb=None, side=64, dev=None, counter=None):
    """The tool's loop: blocks of ``side``^3 voxels, (s + 1)^3 evaluations of ``query(x_obj [n,3]) -> [n]`` per voxel on the
    voxel's own coordinates, +inf outside ``obj_aabb``, one host copy per block -> (occupied [M,3] int64 numpy, resolution)."""
    dev = torch.device("cpu") if dev is None else dev
    aabb_world = aabb_world.to(dev).float()
    R, t, scale = R.to(dev).float(), t.to(dev).float(), scale.to(dev).float()
    resolution = resolution_of(aabb_world, occ_res)
    rl = resolution.tolist()
    out = []
    for (bx, by, bz) in itertools.product(*[range(0, rl[i], side) for i in range(3)]):
        block = [torch.arange(b0, min(b0 + side, rl[i]), device=dev) for i, b0 in enumerate((bx, by, bz))]
        x = voxel_coords(block, resolution, s, aabb_world, R, t, scale, dev)
        xf = x.reshape(-1, 3)
        sdf = torch.full([xf.shape[0]], float("inf"), device=dev)
        if obj_aabb is not None:
            b = obj_aabb.to(dev)
            idx = ((xf >= b[0]) & (xf <= b[1])).all(-1).nonzero()[:, 0]
        else:
            idx = torch.arange(xf.shape[0], device=dev)
        if counter is not None:
            counter[0] += xf.shape[0]
        if idx.shape[0]:
            sdf[idx] = query(xf[idx].contiguous()).reshape(-1).float()
        sdf = sdf.view(x.shape[:-1])
        n_pos = (sdf > 0).sum(dim=-1)
        has = (n_pos < (s + 1) ** 3) & (n_pos > 0) & sdf.isinf().any(dim=-1).logical_not()
        occ = has.nonzero().long() + torch.tensor([bx, by, bz], dtype=torch.long, device=dev)
        out.append(occ.cpu().numpy())
    return np.concatenate(out, axis=0), rl


def sort_rows(a: np.ndarray) -> np.ndarray:
    a = np.asarray(a).reshape(-1, 3).astype(np.int64)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]
