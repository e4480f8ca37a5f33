"""Restatement of ``app/visible_grid.py`` and ``code_multi/tools/extract_visible_grid.py:205-235`` for the tests of
neuralsim_amd/visible_grid.py, in plain torch with separate tensor operations, on dense bool arrays [G, G, G] -- and a loader
of the reference's own class with stand-in modules.  Test infrastructure; the product never imports it."""
import importlib.util
import math
import sys
import types
import typing
from pathlib import Path

import torch
import torch.nn.functional as F

REF_FILE = Path("/root/reference/app/visible_grid.py")


# ------------------------------------------------------------------------------------------------ grid
def grid_of(aabb: torch.Tensor, octree_depth=None, prefer_voxel_size=None):
    """-> (depth, G, origin [3], voxel_size f32 [3]) as the class derives them (visible_grid.py:50, 59-62)"""
    radius3d = (aabb[1] - aabb[0]) / 2.0
    extent = radius3d.max().item() * 2
    depth = octree_depth or math.floor(math.log2(extent / prefer_voxel_size))
    grid_size = aabb.new_tensor([2 ** depth] * 3, dtype=torch.long)
    return depth, 2 ** depth, aabb[0], extent / grid_size


def voxels_of_points(pts: torch.Tensor, aabb: torch.Tensor, depth: int) -> torch.Tensor:
    """flat indices (one per point inside the box, duplicates kept): ``space.contains``, ``((p - origin) / voxel).to(long)``,
    the clamp to G - 1, ``ix G G + iy G + iz``"""
    _, G, origin, voxel = grid_of(aabb, depth)
    inside = ((pts >= aabb[0]) & (pts <= aabb[1])).all(dim=-1)
    p = pts[inside]
    c = ((p - origin) / voxel).to(torch.long).clamp(max=G - 1)
    return (c * c.new_tensor([G * G, G, 1])).sum(-1)


def points_of_samples(rays_o, rays_d, rays_inds_hit, pack_infos_hit, t, w, thre=0.1) -> torch.Tensor:
    """the tool's selection (extract_visible_grid.py:221-226) with the rays addressed through ``rays_inds_hit``"""
    sel = (w > thre).nonzero()[:, 0]
    starts, lens = pack_infos_hit[:, 0].contiguous(), pack_infos_hit[:, 1]
    row = torch.searchsorted(starts, sel, right=True) - 1
    ok = (row >= 0) & (sel < (starts[row.clamp(min=0)] + lens[row.clamp(min=0)]))
    sel, row = sel[ok], row[ok]
    r = rays_inds_hit[row] if rays_inds_hit is not None else row
    d, o = rays_d[r], rays_o[r]
    m = d * t[sel][:, None]
    return o + m


def reduce(indices: torch.Tensor):
    """-> (ascending unique voxels, summed hits)"""
    return indices.unique(return_counts=True)


# ------------------------------------------------------------------------------------------------ morphology
def to_dense(voxels: torch.Tensor, G: int) -> torch.Tensor:
    a = torch.zeros([G * G * G], dtype=torch.bool, device=voxels.device)
    a[voxels] = True
    return a.view(G, G, G)


def to_voxels(dense: torch.Tensor) -> torch.Tensor:
    return dense.reshape(-1).nonzero()[:, 0]


def dilate(a: torch.Tensor) -> torch.Tensor:
    """3x3x3 box dilation, out-of-grid neighbours dropped"""
    return F.max_pool3d(a[None, None].float(), 3, stride=1, padding=1)[0, 0] > 0


def erode(a: torch.Tensor) -> torch.Tensor:
    """3x3x3 box erosion, out-of-grid neighbours empty"""
    return -F.max_pool3d(-F.pad(a[None, None].float(), (1,) * 6, value=0.0), 3, stride=1)[0, 0] > 0


def postprocess(voxels: torch.Tensor, G: int, op: str) -> torch.Tensor:
    orig = to_dense(voxels, G)
    if op == "dilation":
        out = dilate(orig)
    elif op == "close":
        out = erode(dilate(orig)) | orig
    elif op == "close2":
        out = erode(erode(dilate(dilate(orig))) | orig) | orig
    else:
        raise ValueError(op)
    return to_voxels(out)


# ------------------------------------------------------------------------------------------------ the reference's class
class ForestBlockSpace:
    """one block over [0, 1]^3: what the forest branch of the reference's class reads"""

    def __init__(self, device="cpu"):
        self.device = torch.device(device)
        self.world_block_size = torch.ones(3)
        self.world_origin = torch.zeros(3)
        self.n_trees, self.level = 1, 0
        self.block_ks = torch.zeros([1, 3], dtype=torch.long)
        self.spc = types.SimpleNamespace(octrees=None, exsum=None)

    def normalize_coords_01(self, pts):
        inside = ((pts >= 0) & (pts <= 1)).all(dim=-1)
        return pts, torch.where(inside, 0, -1)

    def pidx2blidx(self, pidx):
        return pidx


class AABBSpace:
    pass


class _BoolGridAccel:
    def __init__(self, space=None, resolution=None, **kw):
        G = [int(r) for r in resolution]
        self.occ = types.SimpleNamespace(occ_grid=torch.zeros([space.n_trees, *G], dtype=torch.bool))

    def populate(self):
        pass


def _unbatched_query(octrees, exsum, coords, level, with_parents=False):
    """block (0, 0, 0) of a level-0 forest sits at 0 in [-1, 1]: every other block coordinate leaves that range"""
    return torch.where(((coords >= -1) & (coords < 1)).all(dim=-1), 0, -1)


def load_reference_class():
    """``VisibleGrid`` of the reference, its source unchanged, with stand-ins for kaolin and nr3d_lib"""
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        return m
    log = types.SimpleNamespace(info=lambda *a, **k: None)
    names = dict(Union=typing.Union, Dict=typing.Dict, List=typing.List)
    stubs = {
        "kaolin": mod("kaolin"), "kaolin.ops": mod("kaolin.ops"), "kaolin.ops.spc": mod("kaolin.ops.spc", unbatched_query=_unbatched_query),
        "nr3d_lib": mod("nr3d_lib"), "nr3d_lib.fmt": mod("nr3d_lib.fmt", log=log),
        "nr3d_lib.config": mod("nr3d_lib.config", ConfigDict=dict), "nr3d_lib.models": mod("nr3d_lib.models"),
        "nr3d_lib.models.accelerations": mod("nr3d_lib.models.accelerations", get_accel=lambda type, **kw: _BoolGridAccel(**kw)),
        "nr3d_lib.models.accelerations.occgrid_accel": mod("nr3d_lib.models.accelerations.occgrid_accel",
                                                           OccGridAccel=_BoolGridAccel, OccGridAccelForest=_BoolGridAccel),
        "nr3d_lib.models.attributes": mod("nr3d_lib.models.attributes", **names),
        "nr3d_lib.models.spatial": mod("nr3d_lib.models.spatial", AABBSpace=AABBSpace, ForestBlockSpace=ForestBlockSpace),
    }
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    try:
        spec = importlib.util.spec_from_file_location("_reference_visible_grid", str(REF_FILE))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return m.VisibleGrid


def run_reference(pts: torch.Tensor, depth: int, op: str, save_to=None):
    """the reference's ``reduce_points_and_add -> reduce_voxels -> build_accel -> postprocess(op)`` on one block over [0, 1]^3
    -> (voxels, hits after the reduction, voxels after the post-processing)"""
    g = load_reference_class()(ForestBlockSpace(), depth)
    g.reduce_points_and_add(pts)
    g.reduce_voxels()
    voxels, hits = g.voxels_in_block[0].clone(), g.voxel_hits_in_block[0].clone()
    g.build_accel()
    g.postprocess(op)
    if save_to is not None:
        g.save(save_to)
    return voxels, hits, g.voxels_in_block[0].clone()
