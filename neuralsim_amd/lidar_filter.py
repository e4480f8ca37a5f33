"""Filtering of measured LiDAR sweeps and projection of points into cameras -- the reference's ``SceneDataLoader.filter_lidar_gts``
/ ``_filter_lidar_gts`` (``dataio/data_loader/base_loader.py:649-844``) and ``Camera`` / ``MultiCamBundle.project_pts_in_image``
(``app/resources/observers/cameras.py:397-446, 537-538``), on the kernels ``nsim_lidar_filter_count / _emit`` and
``nsim_cam_project`` (csrc/misc.hip, with ``nsim_occgrid_scan`` between count and emit).

The rule (per point; the reference's four sequential filters are one conjunction; tests/lidar_filter_ref.py restates it in float64):
  * world point  ``p_local = rays_o + rays_d * range`` (one multiply, one add: ``torch.addcmul``), ``p = R p_local + t`` with
    ``(R, t) = l2w[fi][li]``, component k summed as ``((R[k][0] x + R[k][1] y) + R[k][2] z) + t[k]``;
  * ``filter_valid``   keep iff ``range > 0`` (NaN and -0.0 are not kept);
  * ``cams``           keep iff a camera of the point's frame has it in view: ``cam = R_c^T (p - t_c)`` (transposed rotation, no
    inverse), ``(u, v, d)`` by the camera model's ``proj`` (pinhole, OpenCV k1 k2 p1 p2 k3, fisheye k1..k4), in view iff
    ``d > near_clip`` and ``0 <= u < W`` and ``0 <= v < H``, and -- with an ignore mask -- ``ignore[(int)v][(int)u] == 0``;
  * ``aabb``           keep iff ``min <= p <= max`` on every axis;
  * ``boxes``          rows ``[12 floats of a 3x4 transform, 3 sizes]``: keep iff ``b = R_b^T (p - t_b)`` is inside no box,
    inside meaning ``-s / 2 <= b <= s / 2`` on every axis (inclusive).
The kept rows keep the point order.  The host reads ONE number per call, the kept count, from host-mapped words without a stream
synchronisation.  There is no CPU path.

Preconditions the host does not check (each would cost a synchronising read): ``li`` in ``[0, L)`` and ``frame_inds`` in ``[0, F)``
-- a point outside is dropped by the kernel, which reads no table for it; ``frame_offsets`` of a bank describe its rows only when
``frame_inds`` ascend (the kernels themselves take any order; a block of 256 points that shares one frame is the fast case).
"""
import ctypes
from collections import namedtuple
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib

MODELS = {"pinhole": 0, "opencv": 1, "fisheye": 2}
MAX_CAMS = 32                # csrc/misc.hip LF_MAX_CAMS: the model ids of a rig travel as one launch argument
CAM_FLOATS = 24              # csrc/misc.hip LF_CAM
_NOTIFY = None

namedtuple_mask_nuvd = namedtuple("namedtuple_mask_nuvd", "mask n u v d")
namedtuple_mask_niuvd = namedtuple("namedtuple_mask_niuvd", "mask n i u v d")


def _rows34(t: torch.Tensor, name: str, lead: Sequence[int] = None) -> torch.Tensor:
    """a device f32 contiguous [..., 3, 4] / [..., 4, 4] pose tensor -> its contiguous [..., 3, 4] rows"""
    _lib.require_device(t, name)
    if t.dtype != torch.float32:
        raise TypeError(f"lidar_filter: {name} must be float32, got {t.dtype}")
    if t.dim() < 2 or tuple(t.shape[-2:]) not in ((3, 4), (4, 4)) or (lead is not None and t.dim() - 2 not in lead):
        raise ValueError(f"lidar_filter: {name} must be [..., 3, 4] or [..., 4, 4], got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"lidar_filter: {name} must be contiguous")
    return t if t.shape[-2] == 3 else t[..., :3, :].contiguous()


class CameraSet:
    """The cameras of one frame (prefix ``[C]``, or ``()`` for a single camera) or of a sequence (``[F, C]``) as the device table
    the kernels read.  ``c2w`` f32 ``[*prefix, 3, 4]`` / ``[*prefix, 4, 4]`` and ``intr`` f32 ``[*prefix, 3, 3]`` on the device,
    contiguous; ``hw`` = (H, W) per camera (``[*prefix, 2]``, host or device) or one pair for all; ``model`` a name or one per
    camera of the rig; ``distortion`` ``[*prefix, <= 5]`` (missing coefficients are 0); ``downscale`` a scalar or (w, h): the
    intrinsics' rows are multiplied by f32(1 / w), f32(1 / h) and ``W = round(W / w)``, ``H = round(H / h)``, as the intrinsics
    attribute's ``set_downscale`` does."""

    def __init__(self, c2w: torch.Tensor, intr: torch.Tensor, hw, model: Union[str, Sequence[str]] = "pinhole",
                 distortion: torch.Tensor = None, downscale=1):
        c2w = _rows34(c2w, "c2w", lead=(0, 1, 2))
        self.prefix = tuple(c2w.shape[:-2])
        _lib.require_device(intr, "intr")
        if tuple(intr.shape) != (*self.prefix, 3, 3) or intr.dtype != torch.float32:
            raise ValueError(f"lidar_filter: intr must be float32 {[*self.prefix, 3, 3]}, got {intr.dtype} {tuple(intr.shape)}")
        dev = c2w.device
        C = self.prefix[-1] if self.prefix else 1
        F = self.prefix[0] if len(self.prefix) == 2 else 1
        if C > MAX_CAMS:
            raise ValueError(f"lidar_filter: at most {MAX_CAMS} cameras per frame, got {C}")
        names = [model] * C if isinstance(model, str) else list(model)
        if len(names) != C:
            raise ValueError(f"lidar_filter: {len(names)} camera models for {C} cameras")
        for n in names:
            if n not in MODELS:
                raise ValueError(f"lidar_filter: unknown camera model {n!r} (one of {sorted(MODELS)})")
        self.models = [MODELS[n] for n in names]
        self.model_names = names
        hw_t = torch.as_tensor(hw).detach().cpu().to(torch.float32)
        if hw_t.shape[-1:] != (2,) or (hw_t.dim() > 1 and tuple(hw_t.shape[:-1]) != self.prefix):
            raise ValueError(f"lidar_filter: hw must be (H, W) or {[*self.prefix, 2]}, got {tuple(hw_t.shape)}")
        hw_t = hw_t.expand(*self.prefix, 2)
        d = torch.as_tensor(downscale, dtype=torch.float32).reshape(-1)
        dw, dh = float(d[0]), float(d[-1])
        H = torch.round(hw_t[..., 0] / dh)
        W = torch.round(hw_t[..., 1] / dw)
        self.H_max, self.W_max = (int(H.max()), int(W.max())) if H.numel() else (0, 0)
        self.H, self.W = H.long(), W.long()               # host, [*prefix]
        m = intr
        if dw != 1.0 or dh != 1.0:
            m = m * m.new_tensor([1.0 / dw, 1.0 / dh, 1.0])[:, None]
        tab = torch.zeros([*self.prefix, CAM_FLOATS], dtype=torch.float32, device=dev)
        tab[..., :12] = c2w.reshape(*self.prefix, 12)
        tab[..., 12], tab[..., 13], tab[..., 14] = m[..., 0, 0], m[..., 0, 1], m[..., 0, 2]
        tab[..., 15], tab[..., 16] = m[..., 1, 1], m[..., 1, 2]
        tab[..., 17], tab[..., 18] = W.to(dev), H.to(dev)
        if distortion is not None:
            _lib.require_device(distortion, "distortion")
            if tuple(distortion.shape[:-1]) != self.prefix or distortion.shape[-1] > 5:
                raise ValueError(f"lidar_filter: distortion must be {[*self.prefix, '<= 5']}, got {tuple(distortion.shape)}")
            tab[..., 19:19 + distortion.shape[-1]] = distortion.to(torch.float32)
        self.table = tab.reshape(F * C, CAM_FLOATS).contiguous()
        self.C, self.F = C, F
        self.c_models = (ctypes.c_int32 * C)(*self.models) if C else None
        self.device = dev

    @classmethod
    def from_observers(cls, cams: List, downscale=None) -> "CameraSet":
        """From frozen reference ``Camera`` nodes (single frame): ``world_transform``, the intrinsics' unscaled matrix and (H, W)
        with ``downscale`` (default: the one the intrinsics carry), the intrinsics class's ``model``, the ``distortion`` subattr."""
        c2w, mats, hws, names, dist = [], [], [], [], []
        for cam in cams:
            wt = cam.world_transform
            c2w.append((wt.mat_4x4() if hasattr(wt, "mat_4x4") else torch.as_tensor(wt)).detach().to(torch.float32))
            sub = cam.intr.subattr
            mats.append(sub["mat"].tensor.detach().to(torch.float32))
            hws.append(sub["hw"].tensor.detach().cpu().to(torch.float32))
            names.append(getattr(type(cam.intr), "model", "pinhole"))
            dd = sub["distortion"].tensor.detach().to(torch.float32) if "distortion" in sub.keys() else mats[-1].new_zeros(5)
            if dd.shape[-1] > 5 or dd.dim() != 1:
                raise ValueError(f"lidar_filter: camera distortion must be a vector of at most 5 coefficients, got {tuple(dd.shape)}")
            dist.append(torch.cat([dd, dd.new_zeros(5 - dd.shape[-1])]))
            if c2w[-1].shape != (4, 4) or mats[-1].shape != (3, 3):
                raise ValueError("lidar_filter: from_observers takes cameras frozen at a single frame")
        if downscale is None:
            ds = getattr(cams[0].intr, "downscale", 1)
            downscale = ds if not isinstance(ds, tuple) else list(ds)
        return cls(torch.stack(c2w).contiguous(), torch.stack(mats).contiguous(), torch.stack(hws), names,
                   torch.stack(dist).contiguous(), downscale)


def _ignore_u8(ignore_mask: Optional[torch.Tensor], cams: CameraSet, lead: Sequence[int]):
    """-> (u8 [F C, Hm, Wm] or None, Hm, Wm)"""
    if ignore_mask is None:
        return None, 0, 0
    _lib.require_device(ignore_mask, "ignore_mask")
    if ignore_mask.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"lidar_filter: ignore_mask must be bool or uint8, got {ignore_mask.dtype}")
    if tuple(ignore_mask.shape[:-2]) != tuple(lead) or ignore_mask.dim() != len(lead) + 2:
        raise ValueError(f"lidar_filter: ignore_mask must be {[*lead, 'Hm', 'Wm']}, got {tuple(ignore_mask.shape)}")
    Hm, Wm = int(ignore_mask.shape[-2]), int(ignore_mask.shape[-1])
    if Hm < cams.H_max or Wm < cams.W_max:
        raise ValueError(f"lidar_filter: ignore_mask [{Hm}, {Wm}] is smaller than the largest image [{cams.H_max}, {cams.W_max}]"
                         " (pad every mask bottom / right to the same size)")
    if not ignore_mask.is_contiguous():
        raise ValueError("lidar_filter: ignore_mask must be contiguous")
    m = ignore_mask.view(torch.uint8) if ignore_mask.dtype == torch.bool else ignore_mask
    return m.reshape(-1, Hm, Wm), Hm, Wm


def project_pts_in_image(pts: torch.Tensor, cams: CameraSet, ignore_mask: torch.Tensor = None, near_clip: float = 1e-4):
    """``Camera.project_pts_in_image`` (cameras.py:397-446) for world points f32 ``[N, 3]`` (or ``[1, N, 3]``, the reference's
    broadcast form) on the device.  A ``[C]`` camera set -> ``(mask [C, N] bool, n, i, u, v, d)``: the n in-view (and not ignored)
    projections in ``nonzero`` order (camera-major), ``i`` the camera, ``u``, ``v`` int64 pixels, ``d`` f32 depths; a single camera
    (prefix ``()``) -> ``(mask [N], n, u, v, d)``.  ``ignore_mask`` bool / u8 ``[C, Hm, Wm]`` (``[Hm, Wm]``), true = ignored, every
    image padded bottom / right to the same size.  The dense ``[C, N]`` result is the kernel's; its compaction is torch's."""
    _lib.require_device(pts, "pts")
    if len(cams.prefix) == 2:
        raise ValueError("lidar_filter: project_pts_in_image takes the cameras of one frame ([C] or a single camera)")
    if pts.dim() == 3 and pts.shape[0] == 1:
        pts = pts[0]
    if pts.dim() != 2 or pts.shape[-1] != 3 or pts.dtype != torch.float32:
        raise ValueError(f"lidar_filter: pts must be float32 [N, 3] (one point set for all cameras), got {pts.dtype} {tuple(pts.shape)}")
    if not pts.is_contiguous():
        raise ValueError("lidar_filter: pts must be contiguous")
    N, C, dev = int(pts.shape[0]), cams.C, pts.device
    ign, Hm, Wm = _ignore_u8(ignore_mask, cams, cams.prefix)
    mask = torch.empty([C, N], dtype=torch.uint8, device=dev)
    u, v, d = (torch.empty([C, N], dtype=torch.float32, device=dev) for _ in range(3))
    _lib.call("nsim_cam_project", _lib.ptr(pts), N, _lib.ptr(cams.table), cams.c_models, C, float(near_clip), _lib.ptr(ign), Hm, Wm,
              _lib.ptr(mask), _lib.ptr(u), _lib.ptr(v), _lib.ptr(d))
    mask = mask.bool()
    inds = mask.nonzero(as_tuple=True)
    n = int(inds[0].numel())
    if not cams.prefix:
        return namedtuple_mask_nuvd(mask[0], n, u[inds].long(), v[inds].long(), d[inds])
    return namedtuple_mask_niuvd(mask, n, inds[0], u[inds].long(), v[inds].long(), d[inds])


def _notify():
    global _NOTIFY
    if _NOTIFY is None:
        _NOTIFY = _lib.HostNotify(1)
    return _NOTIFY or None


def _column(data: Dict, key: str, N: int, tail, dtype) -> torch.Tensor:
    t = data[key]
    _lib.require_device(t, key)
    if tuple(t.shape) != (N, *tail) or t.dtype != dtype:
        raise ValueError(f"lidar_filter: {key} must be {dtype} {[N, *tail]}, got {t.dtype} {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"lidar_filter: {key} must be contiguous")
    return t


def _filter(data: Dict, fi: Optional[torch.Tensor], l2w: torch.Tensor, F: int, L: int, filter_valid: bool,
            cams: Optional[CameraSet], ign, Hm: int, Wm: int, near_clip: float, aabb: Optional[torch.Tensor],
            boxes: Optional[torch.Tensor], box_offsets: Optional[torch.Tensor], return_inds: bool, return_pts: bool) -> Dict:
    """count -> scan -> emit over flat columns (poses, cameras and masks arrive checked and flattened: l2w [F L, 3, 4], the camera
    table [F C, 24], ign u8 [F C, Hm, Wm]; the columns, the AABB and the boxes are checked here).  -> the filtered dict."""
    global _NOTIFY
    if "ranges" not in data or "rays_o" not in data or "rays_d" not in data:
        raise KeyError("lidar_filter: data needs rays_o, rays_d and ranges")
    _lib.require_device(data["ranges"], "ranges")
    if data["ranges"].dim() != 1:
        raise ValueError(f"lidar_filter: ranges must be [N], got {tuple(data['ranges'].shape)}")
    N, dev = int(data["ranges"].shape[0]), data["ranges"].device
    ranges = _column(data, "ranges", N, (), torch.float32)
    rays_o = _column(data, "rays_o", N, (3,), torch.float32)
    rays_d = _column(data, "rays_d", N, (3,), torch.float32)
    li = _column(data, "li", N, (), torch.long) if "li" in data else None
    extra = [k for k in data if k not in ("rays_o", "rays_d", "ranges", "li")]
    for k in extra:
        v = data[k]
        if not isinstance(v, torch.Tensor) or v.dim() < 1 or v.shape[0] != N:
            raise ValueError(f"lidar_filter: data[{k!r}] must be a tensor with {N} rows")
        _lib.require_device(v, k)
    if aabb is not None:
        _lib.require_device(aabb, "aabb")
        if tuple(aabb.shape) != (2, 3) or aabb.dtype != torch.float32 or not aabb.is_contiguous():
            raise ValueError(f"lidar_filter: aabb must be a contiguous float32 [2, 3] tensor, got {aabb.dtype} {tuple(aabb.shape)}")
    B = 0
    if boxes is not None:
        _lib.require_device(boxes, "boxes")
        if boxes.dim() != 2 or boxes.shape[1] != 15 or boxes.dtype != torch.float32 or not boxes.is_contiguous():
            raise ValueError(f"lidar_filter: boxes must be a contiguous float32 [B, 15] tensor, got {boxes.dtype} {tuple(boxes.shape)}")
        B = int(boxes.shape[0])
        if box_offsets is None:
            if F != 1:
                raise ValueError("lidar_filter: boxes of more than one frame need box_offsets [F + 1]")
            box_offsets = torch.tensor([0, B], dtype=torch.int32).to(dev)
        _lib.require_device(box_offsets, "box_offsets")
        if tuple(box_offsets.shape) != (F + 1,) or box_offsets.dtype != torch.int32 or not box_offsets.is_contiguous():
            raise ValueError(f"lidar_filter: box_offsets must be int32 [{F + 1}], got {box_offsets.dtype} {tuple(box_offsets.shape)}")
    C = cams.C if cams is not None else 0
    M, cnt, keep = 0, None, None
    if N > 0:
        nb = (N + 255) // 256
        keep = torch.empty([N], dtype=torch.uint8, device=dev)
        cnt = torch.empty([nb], dtype=torch.int32, device=dev)
        tot = torch.empty([1], dtype=torch.int32, device=dev)
        _lib.call("nsim_lidar_filter_count", _lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(ranges), _lib.ptr(li), _lib.ptr(fi), N,
                  _lib.ptr(l2w), L, F, int(bool(filter_valid)), _lib.ptr(cams.table if C else None), cams.c_models if C else None, C,
                  float(near_clip), _lib.ptr(ign), Hm, Wm, _lib.ptr(aabb), _lib.ptr(boxes if B else None),
                  _lib.ptr(box_offsets if B else None), B, _lib.ptr(keep), _lib.ptr(cnt))
        nt = _notify()
        adr, seq = nt.arm(0) if nt is not None else (None, 0)
        _lib.call("nsim_occgrid_scan", _lib.ptr(cnt), nb, _lib.ptr(tot), adr, seq)
        M = nt.wait(0, seq) if nt is not None else None
        if M is None:                       # no host-mapped words, or the wait timed out: a synchronising read of the device copy
            M = int(tot.item())
            if nt is not None and int(nt.view[0, 1]) != seq:
                _NOTIFY = False             # finished and still not visible: this memory is not host-coherent
    f32 = dict(dtype=torch.float32, device=dev)
    out = dict(rays_o=torch.empty([M, 3], **f32), rays_d=torch.empty([M, 3], **f32), ranges=torch.empty([M], **f32))
    if li is not None:
        out["li"] = torch.empty([M], dtype=torch.long, device=dev)
    out_fi = torch.empty([M], dtype=torch.long, device=dev) if fi is not None else None
    inds = torch.empty([M], dtype=torch.long, device=dev) if (return_inds or extra) else None
    pts = torch.empty([M, 3], **f32) if return_pts else None
    if M > 0:
        _lib.call("nsim_lidar_filter_emit", _lib.ptr(keep), _lib.ptr(cnt), _lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(ranges),
                  _lib.ptr(li), _lib.ptr(fi), N, _lib.ptr(l2w), L, F, _lib.ptr(out["rays_o"]), _lib.ptr(out["rays_d"]),
                  _lib.ptr(out["ranges"]), _lib.ptr(out.get("li")), _lib.ptr(out_fi), _lib.ptr(inds), _lib.ptr(pts))
    for k in extra:                          # any further per-point column follows the kept indices
        out[k] = data[k][inds]
    out = {k: out[k] for k in data}          # the keys, in the order, of the input
    if out_fi is not None:
        out["frame_inds"] = out_fi
    if return_inds:
        out["keep_inds"] = inds
    if return_pts:
        out["pts_world"] = pts
    return out


def _poses(l2w: torch.Tensor, has_li: bool, bank_frames: Optional[int] = None):
    """-> (l2w [F L, 3, 4], F, L)"""
    m = _rows34(l2w, "l2w", lead=(0, 1) if bank_frames is None else (1, 2))
    if bank_frames is None:
        if m.dim() == 2:
            if has_li:
                raise ValueError("lidar_filter: data carries `li` (a merged sweep) but l2w is a single pose; pass l2w [L, 3, 4]")
            return m.reshape(1, 3, 4), 1, 1
        return m, 1, int(m.shape[0])
    if m.shape[0] != bank_frames:
        raise ValueError(f"lidar_filter: l2w must lead with the {bank_frames} frames, got {tuple(l2w.shape)}")
    if m.dim() == 3:
        if has_li:
            raise ValueError("lidar_filter: data carries `li` (a merged sweep) but l2w has one pose per frame; pass l2w [F, L, 3, 4]")
        return m, bank_frames, 1
    return m.reshape(-1, 3, 4), bank_frames, int(m.shape[1])


def filter_lidar(data: Dict[str, torch.Tensor], l2w: torch.Tensor, *, filter_valid: bool = True, cams: CameraSet = None,
                 ignore_mask: torch.Tensor = None, near_clip: float = 1e-4, aabb: torch.Tensor = None, boxes: torch.Tensor = None,
                 box_offsets: torch.Tensor = None, frame_inds: torch.Tensor = None, return_inds: bool = False,
                 return_pts: bool = False) -> Dict[str, torch.Tensor]:
    """One sweep (``filter_lidar_gts``, base_loader.py:649-844).  ``data``: ``rays_o``, ``rays_d`` f32 [N, 3] and ``ranges`` f32 [N]
    in the lidar's frame, ``li`` int64 [N] for a merged multi-lidar sweep; any further key with N rows is gathered at the kept
    indices.  ``l2w`` f32 [3, 4] / [4, 4], or [L, 3, 4] / [L, 4, 4] with ``li``, contiguous, on the device.  ``cams``: a ``[C]``
    ``CameraSet`` (``filter_in_cams``) with ``ignore_mask`` bool / u8 [C, Hm, Wm]; ``aabb`` f32 [2, 3]; ``boxes`` f32 [B, 15]
    (``filter_out_objs``, the caller picks the classes and the frame).  ``frame_inds`` / ``box_offsets`` belong to
    ``filter_lidar_bank``.  -> the dict with the kept rows in point order (same keys), ``keep_inds`` int64 [M] with ``return_inds``,
    ``pts_world`` f32 [M, 3] with ``return_pts``."""
    if frame_inds is not None:
        raise ValueError("lidar_filter: frame_inds belongs to filter_lidar_bank (filter_lidar takes one frame)")
    if "ranges" in data:
        _lib.require_device(data["ranges"], "ranges")
    m, F, L = _poses(l2w, "li" in data)
    ign, Hm, Wm = None, 0, 0
    if cams is not None:
        if len(cams.prefix) == 2:
            raise ValueError("lidar_filter: filter_lidar takes the cameras of one frame; a [F, C] set belongs to filter_lidar_bank")
        ign, Hm, Wm = _ignore_u8(ignore_mask, cams, cams.prefix)
    elif ignore_mask is not None:
        raise ValueError("lidar_filter: ignore_mask needs cams")
    return _filter(data, None, m, F, L, filter_valid, cams, ign, Hm, Wm, near_clip, aabb, boxes, box_offsets, return_inds,
                   return_pts)


def filter_lidar_bank(frames, l2w: torch.Tensor, *, filter_valid: bool = True, cams: CameraSet = None,
                      ignore_mask: torch.Tensor = None, near_clip: float = 1e-4, aabb: torch.Tensor = None, boxes=None,
                      box_offsets: torch.Tensor = None, frame_inds: torch.Tensor = None, return_inds: bool = False,
                      return_pts: bool = False) -> Dict[str, torch.Tensor]:
    """A whole sequence in ONE count / scan / emit pass.  ``frames``: a list of F per-frame dicts (concatenated here), or one flat
    dict with ``frame_inds`` int64 [N] (argument, or key of the dict), ascending.  ``l2w`` f32 [F, 3, 4] (or [F, L, 3, 4] with
    ``li``); ``cams`` a ``[F, C]`` ``CameraSet`` with ``ignore_mask`` [F, C, Hm, Wm]; ``boxes`` a list of F per-frame f32 [B_f, 15]
    tensors, or one flat [B, 15] tensor with ``box_offsets`` int32 [F + 1].  -> the flat filtered bank: the columns, ``frame_inds``
    [M], ``frame_offsets`` int64 [F + 1] (rows of frame f are ``frame_offsets[f] : frame_offsets[f + 1]``), ``keep_inds`` /
    ``pts_world`` on request (indices into the concatenated input)."""
    if isinstance(frames, (list, tuple)):
        if not frames:
            raise ValueError("lidar_filter: filter_lidar_bank needs at least one frame")
        keys = list(frames[0].keys())
        for fr in frames:
            if list(fr.keys()) != keys:
                raise ValueError("lidar_filter: every frame of a bank carries the same keys")
        for fr in frames:
            _lib.require_device(fr["ranges"], "ranges")
        data = {k: torch.cat([fr[k] for fr in frames]).contiguous() for k in keys}
        sizes = torch.tensor([int(fr["ranges"].shape[0]) for fr in frames], dtype=torch.long)
        F = len(frames)
        fi = torch.repeat_interleave(torch.arange(F, dtype=torch.long), sizes).to(data["ranges"].device)
    else:
        data = dict(frames)
        fi = frame_inds if frame_inds is not None else data.pop("frame_inds", None)
        data.pop("frame_inds", None)
        if fi is None:
            raise ValueError("lidar_filter: a flat bank needs frame_inds")
        F = int(l2w.shape[0]) if isinstance(l2w, torch.Tensor) and l2w.dim() >= 3 else 0
        _lib.require_device(fi, "frame_inds")
        if fi.dtype != torch.long or fi.dim() != 1 or not fi.is_contiguous() or fi.shape[0] != data["ranges"].shape[0]:
            raise ValueError(f"lidar_filter: frame_inds must be a contiguous int64 [N] tensor, got {fi.dtype} {tuple(fi.shape)}")
    m, F, L = _poses(l2w, "li" in data, bank_frames=F)
    dev = data["ranges"].device
    ign, Hm, Wm = None, 0, 0
    if cams is not None:
        if len(cams.prefix) != 2 or cams.F != F:
            raise ValueError(f"lidar_filter: a bank of {F} frames takes a [{F}, C] camera set, got prefix {list(cams.prefix)}")
        ign, Hm, Wm = _ignore_u8(ignore_mask, cams, cams.prefix)
    elif ignore_mask is not None:
        raise ValueError("lidar_filter: ignore_mask needs cams")
    if isinstance(boxes, (list, tuple)):
        if len(boxes) != F:
            raise ValueError(f"lidar_filter: {len(boxes)} box lists for {F} frames")
        offs = np.concatenate([[0], np.cumsum([int(b.shape[0]) for b in boxes])]).astype(np.int32)
        box_offsets = torch.from_numpy(offs).to(dev)
        boxes = torch.cat([b.reshape(-1, 15) for b in boxes]).contiguous()
    out = _filter(data, fi, m, F, L, filter_valid, cams, ign, Hm, Wm, near_clip, aabb, boxes, box_offsets, return_inds, return_pts)
    counts = torch.bincount(out["frame_inds"], minlength=F)[:F]
    out["frame_offsets"] = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)])
    return out


# ------------------------------------------------------------------------------------------------ the reference's loader
def reference_filter_adapter(loader, data: Dict[str, torch.Tensor], pts: torch.Tensor, frozen_scene, *, filter_valid=True,
                             filter_in_cams=False, filter_out_objs=False, filter_out_obj_dynamic_only=False,
                             filter_out_obj_classnames: List[str] = None, filter_in_aabb: torch.Tensor = None, inplace=False):
    """``SceneDataLoader._filter_lidar_gts`` (base_loader.py:732-844), signature and return value, on the fused pass.  ``pts`` are
    the world points the caller computed: they enter as the rays (origin ``pts``, direction 0, identity pose), so the kernel's world
    point is ``pts`` bit for bit; the columns of ``data`` follow the kept indices.  Cameras: ``frozen_scene.observers[...]`` of
    ``loader.cam_id_list`` at ``loader.config.tags.camera.downscale``; ignore masks: ``loader.get_image_ignore_mask`` when
    ``image_ignore_mask`` is configured, padded bottom / right; boxes: ``frozen_scene.metas`` at ``frame_ind + data_frame_offset``
    for ``filter_out_obj_classnames``.  ``NSIM_LIDAR_FILTER=hip`` (tools/run_reference_train.py) installs it on the class."""
    assert frozen_scene.i is not None, "scene needs to be frozen in advance."
    frame_ind = int(frozen_scene.i)
    dev = pts.device
    cams = ign = boxes = None
    if filter_in_cams:
        cam_id_list = loader.cam_id_list
        cams = CameraSet.from_observers([frozen_scene.observers[cid] for cid in cam_id_list],
                                        downscale=loader.config.tags.camera.downscale)
        if "image_ignore_mask" in loader.config.tags:
            masks = [loader.get_image_ignore_mask(scene_id=frozen_scene.id, cam_id=cid, frame_ind=frame_ind, device=loader.device)
                     for cid in cam_id_list]
            Hm = max(max(int(mk.shape[0]) for mk in masks), cams.H_max)
            Wm = max(max(int(mk.shape[1]) for mk in masks), cams.W_max)
            ign = torch.zeros([len(masks), Hm, Wm], dtype=torch.bool, device=dev)
            for k, mk in enumerate(masks):
                ign[k, :mk.shape[0], :mk.shape[1]] = mk.to(dev)
    if filter_out_objs:
        assert "obj_box_list_per_frame" in frozen_scene.metas.keys()
        key = "obj_box_list_per_frame_dynamic_only" if filter_out_obj_dynamic_only else "obj_box_list_per_frame"
        obj_box_list = frozen_scene.metas[key]
        class_names = filter_out_obj_classnames or list(obj_box_list.keys())
        k = frame_ind + frozen_scene.data_frame_offset
        rows = [np.asarray(obj_box_list[c][k]).reshape(-1, 15) if (c in obj_box_list) and (len(obj_box_list[c][k]) > 0)
                else np.empty([0, 15]) for c in class_names]
        rows = np.concatenate(rows, axis=0)
        if len(rows) > 0:
            boxes = torch.tensor(rows, dtype=torch.float, device=dev)
    if filter_in_aabb is not None:
        assert isinstance(filter_in_aabb, torch.Tensor) and list(filter_in_aabb.shape) == [2, 3], \
            f"Invalid filter_in_aabb={filter_in_aabb}"
        filter_in_aabb = filter_in_aabb.to(device=dev, dtype=torch.float32).contiguous()
    N = int(pts.shape[0])
    cols = dict(rays_o=pts.reshape(N, 3).to(torch.float32).contiguous(), rays_d=torch.zeros([N, 3], dtype=torch.float32, device=dev),
                ranges=data["ranges"].to(torch.float32).contiguous())
    eye = torch.eye(4, dtype=torch.float32, device=dev)[:3].contiguous()
    ret = filter_lidar(cols, eye, filter_valid=filter_valid, cams=cams, ignore_mask=ign, aabb=filter_in_aabb, boxes=boxes,
                       return_inds=True)
    inds = ret["keep_inds"]
    out = data if inplace else data.copy()
    for k in list(out.keys()):
        out[k] = out[k][inds]
    return out
