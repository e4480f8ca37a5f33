"""Visible grids: the voxels the training cameras actually saw (``app/visible_grid.py`` ``VisibleGrid`` and
``code_multi/tools/extract_visible_grid.py:205-235``), marked, closed and compacted on the device (csrc/misc.hip ``nsim_vgrid_*``).

Semantics (the reference's, restated; tests/visible_grid_ref.py restates them once more in plain torch):
  * ``octree_depth = octree_depth or floor(log2(grid_extent / prefer_voxel_size))``, ``grid_size = [2^depth] * 3``,
    ``grid_extent = space.radius3d.max() * 2``, ``voxel_size = grid_extent / grid_size`` (cubic voxels);
  * every volume-render sample with ``vw_normalized > 0.1`` of every hit ray gives the point ``rays_o + rays_d * t``; points with
    ``space.contains(p)`` count, at voxel ``((p - origin) / voxel_size).to(long)``, flat index ``ix G G + iy G + iz``;
  * ``reduce_voxels``: the ascending unique indices over all calls, with the hit counts;
  * ``postprocess(op)`` on the 26-neighbourhood, with D = 3x3x3 dilation (out-of-grid neighbours dropped), E = 3x3x3 erosion
    (out-of-grid neighbours empty) and ``orig`` the set before: ``dilation`` D(orig), ``close`` E(D(orig)) | orig,
    ``close2`` E(E(D(D(orig))) | orig) | orig;
  * the file: ``torch.save({"octree_depth": int, "voxels_in_block": {0: int64 [M]}})``.
Where this class departs from the reference's (which does not run for an ``AABBSpace``): the origin ``grid_center`` is the box's
minimum corner, the grid is the cube ``[origin, origin + grid_extent]`` and the accel is built over that cube, coordinates are
clamped to G - 1, rays are addressed through ``rays_inds_hit``, hit counts are summed over all calls, and a ``ForestBlockSpace``
raises ``NotImplementedError`` (DESIGN.md section 7 lists each with its file:line).

The working grids -- hit counts int32 [G^3], bit sets uint32 [G^3 / 32] -- are kept in the REFERENCE's voxel order (z fastest), so
the compaction emits ``voxels_in_block`` ascending without a sort and the morphology packs z into the words.  The accel's order is
x fastest: the one transposition happens where the bits are written into the accel's value grid (``nsim_vgrid_occ_val``), after
which the accel's own ``pack_bits`` runs.
"""
import math
from typing import Dict, Optional

import torch

from . import _lib
from .fields.neus import OccGridAccel
from .spatial import make_occ_meta

MIN_DEPTH, MAX_DEPTH = 5, 10
_DILATE, _ERODE = 0, 1


def voxel_indices_to_voxel_coords(voxel_indices: torch.Tensor, grid_size: torch.Tensor):
    strides = grid_size.new_tensor([grid_size[1] * grid_size[2], grid_size[2], 1])
    coord_x = voxel_indices // strides[0]
    coord_y = (voxel_indices - coord_x * strides[0]) // strides[1]
    coord_z = voxel_indices % strides[1]
    return torch.stack([coord_x, coord_y, coord_z], 1)


def voxel_coords_to_voxel_indices(voxel_coords: torch.Tensor, grid_size: torch.Tensor):
    strides = grid_size.new_tensor([grid_size[1] * grid_size[2], grid_size[2], 1])
    return (voxel_coords * strides).sum(-1)


class VisibleGridAccel(OccGridAccel):
    """The occupancy accel of a visible grid: G^3 cells over the grid's cube (``meta``, ``grid_aabb``), value 1.0 in a visible
    voxel and 0.0 elsewhere, threshold 0.5.  ``aabb`` stays the SPACE's box -- a model reads its own box from ``accel.aabb`` -- and
    ``box_meta`` is the ray-test form of it; for a cubic space the two boxes coincide.  No training hook refreshes it."""

    def __init__(self, space_aabb: torch.Tensor, grid_aabb: torch.Tensor, G: int, device=None):
        super().__init__(space_aabb, resolution=[G] * 3, occ_thre=0.5, update_from_samples_cfg=None, device=device)
        self.register_buffer("grid_aabb", grid_aabb.detach().float().reshape(2, 3).clone().to(self.aabb.device))
        self.meta = self._make_meta()
        self.box_meta = make_occ_meta(self.aabb.detach().cpu())

    def _make_meta(self):
        m = _lib.OccMeta()
        a = getattr(self, "grid_aabb", self.aabb).detach().cpu()
        scale = torch.tensor(self.resolution, dtype=torch.float32) / (a[1] - a[0])
        for i in range(3):
            m.aabb_min[i], m.aabb_max[i] = float(a[0, i]), float(a[1, i])
            m.scale[i] = float(scale[i])
            m.res[i] = self.resolution[i]
        return m

    def update_from_net(self, *a, **k):
        pass

    def update_from_samples(self, *a, **k):
        pass

    def collect(self, *a, **k):
        pass

    def init(self, *a, **k):
        pass

    def cur_batch__step(self, *a, **k):
        pass


class VisibleGrid:
    def __init__(self, space, octree_depth: int = None, prefer_voxel_size: float = None) -> None:
        if type(space).__name__ == "ForestBlockSpace":
            raise NotImplementedError("VisibleGrid: ForestBlockSpace is not supported (the forest model is not built here)")
        if not (hasattr(space, "aabb") and hasattr(space, "contains")):
            raise NotImplementedError("Only support AABBSpace now")
        _lib.require_device(space.aabb, "space.aabb")
        self.space = space
        self.accel = None
        self.grid_center = space.aabb[0].detach().clone()           # the grid's minimum corner (the name is the reference's)
        self.grid_extent_in_world = self.grid_extent = space.radius3d.max().item() * 2
        if not octree_depth:
            if not prefer_voxel_size or prefer_voxel_size <= 0:
                raise ValueError("VisibleGrid: give octree_depth or a positive prefer_voxel_size")
            octree_depth = math.floor(math.log2(self.grid_extent / prefer_voxel_size))
        self.octree_depth = int(octree_depth)
        if not MIN_DEPTH <= self.octree_depth <= MAX_DEPTH:
            raise ValueError(f"VisibleGrid: octree_depth must be {MIN_DEPTH}..{MAX_DEPTH}, got {self.octree_depth}")
        self.grid_size = self.grid_center.new_tensor([2 ** self.octree_depth] * 3, dtype=torch.long)
        self.voxel_size = self.grid_extent / self.grid_size
        self.voxel_size_in_world = self.grid_extent_in_world / self.grid_size
        self.voxels_in_block: Dict[int, torch.Tensor] = {}
        self.voxel_hits_in_block: Dict[int, torch.Tensor] = {}
        self._hits = None                 # int32 [G^3], allocated by the first marking call
        self._occ = None                  # the accel's voxels as a bit set (build_accel)
        a, v = space.aabb.detach().cpu().float(), self.voxel_size.detach().cpu().float()
        f = _lib.VgridFrame()
        f.G = self.G
        for i in range(3):
            f.origin[i], f.voxel[i] = float(a[0, i]), float(v[i])
            f.box_min[i], f.box_max[i] = float(a[0, i]), float(a[1, i])
        self._frame = f

    # ------------------------------------------------------------------ sizes
    @property
    def G(self) -> int:
        return 1 << self.octree_depth

    @property
    def device(self):
        return self.grid_center.device

    def _new_bits(self, zero: bool = True) -> torch.Tensor:
        n = self.G ** 3 // 32
        return (torch.zeros if zero else torch.empty)([n], dtype=torch.int32, device=self.device)

    def _hits_grid(self) -> torch.Tensor:
        if self._hits is None:
            self._hits = torch.zeros([self.G ** 3], dtype=torch.int32, device=self.device)
        return self._hits

    # ------------------------------------------------------------------ file
    @staticmethod
    def load(file_path: str, space):
        state_dict = torch.load(file_path, map_location=space.aabb.device, weights_only=False)
        visible_grid = VisibleGrid(space, state_dict["octree_depth"])
        visible_grid.voxels_in_block = {k: v.to(space.aabb.device).long() for k, v in state_dict["voxels_in_block"].items()}
        return visible_grid

    def save(self, file: str):
        torch.save({
            "octree_depth": self.octree_depth,
            "voxels_in_block": dict(self.voxels_in_block)
        }, file)

    # ------------------------------------------------------------------ marking
    @torch.no_grad()
    def add_samples(self, rays_o: torch.Tensor, rays_d: torch.Tensor, volume_buffer: Optional[dict] = None, *,
                    vw_normalized: torch.Tensor = None, t: torch.Tensor = None, pack_infos_hit: torch.Tensor = None,
                    rays_inds_hit: torch.Tensor = None, thre: float = 0.1, stats: torch.Tensor = None):
        """The fused path: every sample with ``vw_normalized > thre`` of a packed volume buffer (``volume_buffer``, or its fields
        ``vw_normalized``, ``t`` [S], ``pack_infos_hit`` [R',2], ``rays_inds_hit`` [R'] -- None: row p of the pack infos is ray
        p) marks the voxel of ``rays_o[r] + rays_d[r] * t``; no selection list, no point array.  ``rays_o`` / ``rays_d`` [R,3] are
        the rays ``rays_inds_hit`` indexes.  ``stats``: int64 [2] on the device, += (samples counted, atomics issued)."""
        if volume_buffer is not None:
            if volume_buffer.get("type", "packed") == "empty":
                return
            if volume_buffer.get("type", "packed") != "packed":
                raise NotImplementedError("VisibleGrid.add_samples: packed volume buffers only")
            vw_normalized, t = volume_buffer["vw_normalized"], volume_buffer["t"]
            pack_infos_hit, rays_inds_hit = volume_buffer["pack_infos_hit"], volume_buffer.get("rays_inds_hit")
        if vw_normalized is None or t is None or pack_infos_hit is None:
            raise ValueError("VisibleGrid.add_samples: needs a volume buffer or vw_normalized, t and pack_infos_hit")
        tensors = dict(rays_o=rays_o, rays_d=rays_d, vw_normalized=vw_normalized, t=t, pack_infos_hit=pack_infos_hit)
        if rays_inds_hit is not None:
            tensors["rays_inds_hit"] = rays_inds_hit
        for k, v in tensors.items():
            _lib.require_device(v, k)
        o, d = rays_o.detach().float().contiguous(), rays_d.detach().float().contiguous()
        w, tt = vw_normalized.detach().float().contiguous().view(-1), t.detach().float().contiguous().view(-1)
        pi = pack_infos_hit.long().contiguous()
        ri = rays_inds_hit.long().contiguous() if rays_inds_hit is not None else None
        if o.dim() != 2 or o.shape[1] != 3 or d.shape != o.shape:
            raise ValueError("VisibleGrid.add_samples: rays_o and rays_d must be [R,3]")
        if w.shape != tt.shape or pi.dim() != 2 or pi.shape[1] != 2 or (ri is not None and ri.shape[0] != pi.shape[0]):
            raise ValueError("VisibleGrid.add_samples: vw_normalized and t are [S], pack_infos_hit [R',2], rays_inds_hit [R']")
        _lib.call("nsim_vgrid_mark_samples", self._frame, _lib.ptr(o), _lib.ptr(d), o.shape[0], _lib.ptr(ri), _lib.ptr(pi),
                  pi.shape[0], _lib.ptr(tt), _lib.ptr(w), w.shape[0], float(thre), _lib.ptr(self._hits_grid()), _lib.ptr(stats))

    def _voxels_of(self, pts: torch.Tensor) -> torch.Tensor:
        """the reference's tensor expression (visible_grid.py:88, 119-120) + the clamp: flat indices of the points inside"""
        pts = pts[self.space.contains(pts)]
        voxel_coords = ((pts - self.grid_center) / self.voxel_size).to(torch.long).clamp(max=self.G - 1)
        return voxel_coords_to_voxel_indices(voxel_coords, self.grid_size)

    @torch.no_grad()
    def reduce_points_and_add(self, pts: torch.Tensor, return_frame: bool = False, stats: torch.Tensor = None):
        """Mark the voxels of ``pts`` [n,3].  ``return_frame=True`` (a debugging aid, through ``torch.unique``): this call's
        ``({0: voxels}, {0: hits})``, as the reference returns them."""
        _lib.require_device(pts, "pts")
        pts = pts.detach().float().reshape(-1, 3).contiguous()
        _lib.call("nsim_vgrid_mark_points", self._frame, _lib.ptr(pts), pts.shape[0], _lib.ptr(self._hits_grid()), _lib.ptr(stats))
        if return_frame:
            voxels, hits = self._voxels_of(pts).unique(return_counts=True)
            return {0: voxels}, {0: hits}
        return None

    # ------------------------------------------------------------------ bit sets <-> index lists
    def _compact(self, bits: torch.Tensor, with_hits: bool):
        """bit set -> (ascending int64 indices, hit counts at them or None): count -> scan -> emit, no atomics"""
        dev, G = bits.device, self.G
        nb = (G ** 3 // 32 + 255) // 256
        cnt = torch.empty([nb], dtype=torch.int32, device=dev)
        tot = torch.empty([1], dtype=torch.int32, device=dev)
        _lib.call("nsim_vgrid_count", _lib.ptr(bits), G, _lib.ptr(cnt))
        _lib.call("nsim_occgrid_scan", _lib.ptr(cnt), nb, _lib.ptr(tot), None, 0)
        m = int(tot.item())                                   # the one size read of a compaction
        idx = torch.empty([m], dtype=torch.int64, device=dev)
        hits = torch.empty([m], dtype=torch.int64, device=dev) if with_hits else None
        if m > 0:
            _lib.call("nsim_vgrid_emit", _lib.ptr(bits), G, _lib.ptr(cnt), _lib.ptr(self._hits), _lib.ptr(idx), _lib.ptr(hits))
        return idx, hits

    def _bits_of(self, voxels: Optional[torch.Tensor]) -> torch.Tensor:
        bits = self._new_bits()
        if voxels is not None and voxels.numel():
            _lib.require_device(voxels, "voxels_in_block")
            v = voxels.long().contiguous()
            _lib.call("nsim_vgrid_set_bits", _lib.ptr(v), v.shape[0], self.G, _lib.ptr(bits))
        return bits

    @torch.no_grad()
    def reduce_voxels(self):
        """``voxels_in_block[0]``: the ascending indices of every voxel marked so far, ``voxel_hits_in_block[0]``: how many points
        each has seen, summed over all calls."""
        if self._hits is None and 0 in self.voxels_in_block:      # a loaded grid nothing was added to
            return self
        bits = self._new_bits(zero=False)
        _lib.call("nsim_vgrid_bits", _lib.ptr(self._hits_grid()), self.G, _lib.ptr(bits))
        self.voxels_in_block[0], self.voxel_hits_in_block[0] = self._compact(bits, True)
        return self

    # ------------------------------------------------------------------ accel and morphology
    def _push(self):
        _lib.call("nsim_vgrid_occ_val", _lib.ptr(self._occ), self.G, _lib.ptr(self.accel.occ_val))
        self.accel.pack_bits()

    @torch.no_grad()
    def build_accel(self):
        cube = torch.stack([self.grid_center, self.grid_center + self.grid_extent])
        self.accel = VisibleGridAccel(self.space.aabb.detach(), cube, self.G, device=self.device)
        self._occ = self._bits_of(self.voxels_in_block.get(0))
        self._push()
        return self

    def _need_accel(self, what: str):
        if self.accel is None or self._occ is None:
            raise RuntimeError(f"VisibleGrid.{what}: call build_accel() first")

    def _morph(self, src: torch.Tensor, keep: Optional[torch.Tensor], op: int) -> torch.Tensor:
        out = self._new_bits(zero=False)
        _lib.call("nsim_vgrid_morph", _lib.ptr(src), _lib.ptr(keep), self.G, op, _lib.ptr(out))
        return out

    @torch.no_grad()
    def dilation_occ_grid(self):
        """the accel's grid |= the 26-neighbourhood of ``voxels_in_block`` (visible_grid.py:166-177)"""
        self._need_accel("dilation_occ_grid")
        self._occ = self._morph(self._bits_of(self.voxels_in_block.get(0)), self._occ, _DILATE)
        self._push()

    @torch.no_grad()
    def erosion_occ_grid(self):
        """the accel's grid = its erosion | ``voxels_in_block`` (visible_grid.py:179-201)"""
        self._need_accel("erosion_occ_grid")
        self._occ = self._morph(self._occ, self._bits_of(self.voxels_in_block.get(0)), _ERODE)
        self._push()

    @torch.no_grad()
    def update_voxels_in_block_from_occgrid(self):
        self._need_accel("update_voxels_in_block_from_occgrid")
        idx, hits = self._compact(self._occ, self._hits is not None)
        self.voxels_in_block = {0: idx}
        self.voxel_hits_in_block = {0: hits} if hits is not None else {}
        return self

    @torch.no_grad()
    def postprocess(self, morphology_op="close"):
        assert morphology_op == "dilation" or morphology_op == "close" or morphology_op == "close2", \
            "Only support dilation, close, close2 operation"
        self._need_accel("postprocess")
        # the reference's sequence (visible_grid.py:217-232) with the pushes to the accel folded into one at the end
        orig = self._bits_of(self.voxels_in_block.get(0))
        occ = self._morph(orig, self._occ, _DILATE)
        if morphology_op == "close2":
            occ = self._morph(occ, occ, _DILATE)
        if morphology_op == "close" or morphology_op == "close2":
            if morphology_op == "close2":
                occ = self._morph(occ, orig, _ERODE)
            occ = self._morph(occ, orig, _ERODE)
        self._occ = occ
        self._push()
        return self.update_voxels_in_block_from_occgrid()

    # ------------------------------------------------------------------ geometry
    def get_grid_center_in_world(self, block_index: int = 0):
        return self.grid_center

    def get_grid_aabb_in_world(self, block_index: int = 0):
        grid_min = self.get_grid_center_in_world(block_index)
        grid_max = grid_min + self.grid_extent_in_world
        return grid_min, grid_max

    def get_voxel_aabb_in_world(self, voxel_indices: torch.Tensor, block_index: int = 0):
        voxel_coords = voxel_indices_to_voxel_coords(voxel_indices, self.grid_size)
        voxel_mins = voxel_coords * self.voxel_size_in_world + \
            self.get_grid_center_in_world(block_index)
        voxel_maxs = voxel_mins + self.voxel_size_in_world
        return voxel_mins, voxel_maxs


# ------------------------------------------------------------------------------------------------ driver
def infer_voxel_size(intr: torch.Tensor, far: float, downscale: float = 1.0) -> float:
    """The tool's inference (extract_visible_grid.py:74-84): twice the gap between neighbouring rays at the far plane,
    ``2 * far * max over cameras of ||1 / focal||`` with the focal lengths of the down-scaled images."""
    focal = torch.stack([intr[..., 0, 0], intr[..., 1, 1]], dim=-1).reshape(-1, 2).float() / float(downscale)
    gap = float((1.0 / focal).norm(dim=-1).max())
    return gap * float(far) * 2.0


def normalized_visibility(alpha: torch.Tensor, pack_infos: torch.Tensor) -> torch.Tensor:
    """``vw_normalized`` of a packed buffer (buffer_compose_renderer.py:699-701)"""
    from .graphics import pack_ops as po
    vw = po.packed_alpha_to_vw(alpha, pack_infos)
    return po.packed_div(vw, po.packed_sum(vw, pack_infos) + 1e-10, pack_infos)


def view_buffers(renderer_or_model, rays_o, rays_d, *, model=None, near=None, far=None, forward_inv_s=64000.):
    """The packed volume buffer of one ray chunk with ``vw_normalized`` filled in, or None when nothing was hit."""
    if hasattr(renderer_or_model, "ray_test"):
        m = renderer_or_model
        tested = m.ray_test(rays_o, rays_d, near=near, far=far)
        cfg = dict(m.ray_query_cfg)
        cfg.update(with_rgb=False, with_normal=False, perturb=False, forward_inv_s=forward_inv_s)
        vb = m.ray_query(ray_tested=tested, config=cfg, return_buffer=True)["volume_buffer"]
    else:
        if model is None:
            raise ValueError("visible_grid: a renderer needs model=")
        ret = renderer_or_model.ray_query(rays_o, rays_d, model=model, near=near, far=far, with_rgb=False, with_normal=False,
                                          return_buffer=True, bypass_ray_query_cfg=dict(forward_inv_s=forward_inv_s, perturb=False))
        vb = ret["volume_buffer"]
    if vb["type"] == "empty":
        return None
    if "vw_normalized" not in vb:
        vb = dict(vb, vw_normalized=normalized_visibility(vb["opacity_alpha"].detach(), vb["pack_infos_hit"]))
    return vb


@torch.no_grad()
def visible_grid_from_views(renderer_or_model, intr, c2w, WH, frames, *, model=None, rayschunk: int = 4096,
                            forward_inv_s: float = 64000., vw_thre: float = 0.1, voxel_size: float = None,
                            octree_depth: int = None, downscale: float = 1.0, near=None, far=None, distortion=None) -> VisibleGrid:
    """Render the views ``frames`` (indices into ``intr`` [V,3,3], ``c2w`` [V,4,4], ``WH`` [V,2]) in chunks of ``rayschunk`` rays
    without gradients, feed every chunk's volume buffer to ``VisibleGrid.add_samples`` and reduce: the tool's loop
    (extract_visible_grid.py:205-235).  ``renderer_or_model``: a NeuS model, or a single-volume renderer with ``model=``.
    Neither ``voxel_size`` nor ``octree_depth``: ``infer_voxel_size`` (needs ``far``, or the renderer's)."""
    from .eval import all_pixel_xy
    from .graphics.cameras import selected_rays
    m = renderer_or_model if hasattr(renderer_or_model, "ray_test") else model
    if m is None:
        raise ValueError("visible_grid: a renderer needs model=")
    if far is None and not hasattr(renderer_or_model, "ray_test"):
        far = renderer_or_model.config.get("far", None)
    if not voxel_size and not octree_depth:
        if far is None:
            raise ValueError("visible_grid: inferring the voxel size needs far")
        voxel_size = infer_voxel_size(intr, far, downscale)
    grid = VisibleGrid(m.space, octree_depth=octree_depth, prefer_voxel_size=voxel_size)
    for frame in frames:
        W, H = max(1, int(int(WH[frame, 0]) / downscale)), max(1, int(int(WH[frame, 1]) / downscale))
        xy = all_pixel_xy(W, H, intr.device)
        fidx = torch.full([xy.shape[0]], int(frame), dtype=torch.long, device=intr.device)
        rays_o, rays_d = selected_rays(xy, fidx, intr, c2w, WH, distortion=distortion)
        for i in range(0, rays_o.shape[0], int(rayschunk)):
            o, d = rays_o[i:i + rayschunk].contiguous(), rays_d[i:i + rayschunk].contiguous()
            vb = view_buffers(renderer_or_model, o, d, model=model, near=near, far=far, forward_inv_s=forward_inv_s)
            if vb is not None:
                grid.add_samples(o, d, vb, thre=vw_thre)
    return grid.reduce_voxels()
