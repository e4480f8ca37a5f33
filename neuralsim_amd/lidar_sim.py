"""Simulated LiDAR sensors: beam-pattern ray generation and the point cloud a rendered sweep delivers -- the reference's
``Lidar`` observer node (``app/resources/observers/lidars.py:177-588``) and what the tools do with it
(``code_multi/tools/render.py:236-355``, ``render_anim.py:198-330``, ``manipulate.py:438-470``,
``extract_visible_grid.py:97-131``), on the kernels ``nsim_lidar_raygen`` (csrc/sampling.hip) and
``nsim_lidar_returns_count / _emit`` (csrc/misc.hip, with ``nsim_occgrid_scan`` between them).

Angles and rays (the node's, restated; tests/lidar_sim_ref.py restates them once more in float64):
  * ``theta`` is the polar angle from the sensor's z axis, ``phi`` the azimuth; a *grid* sensor (spinning units) fires every beam
    ``thetas[j]`` at every azimuth ``phis[i]``, ray ``r = i n_beams + j`` (beam fastest: the flatten order of
    ``torch.meshgrid(thetas, phis, indexing='xy')``); a *paired* sensor (solid-state and Risley-prism scan patterns) fires ray r at
    ``(thetas[r], phis[r])``;
  * ``d = normalize(sinT cosP X + sinT sinP Y + cosT Z)`` with X, Y, Z the columns of ``l2w`` = ``world_transform x
    carla_to_opencv``; ``axis=1`` is the variant the reference uses for its ``bpearl`` unit, ``cosT X + sinT sinP Y - sinT cosP Z``;
    the origin is the translation column for every ray.

Sensor-description files (``load_sensor_specs``).  The package ships NO vendor beam tables: a user supplies them.  A file is JSON
(``.json``) or a ``torch.save``d object (anything else) holding ``{"sensors": [entry, ...]}`` (or the list alone); an entry is
    ``lidar_model``  str   the generator family, as ``--lidar_model`` names it (``Surround``, ``Solid_state``, ``Risley_prism`` ...)
    ``lidar_name``   str   the unit, as ``--lidar_id`` names it; (lidar_model, lidar_name) is the key of the returned dict
    ``mode``         "grid" | "paired"      (default "grid")
    ``axis``         0 | 1                  (default 0)
    ``near``, ``far``      metres           (defaults 0.3 and 120.0, the node's)
    ``rolling_shutter_effect``  bool        (default false; per-beam timestamps are not implemented, as in the reference)
and the angles, one of
    ``thetas`` + ``phis``              radians, numbers or tensors (f32 tensors are taken bit for bit)
    ``elevations_deg`` + ``phis``      ``thetas = pi / 2 - elev pi / 180`` evaluated in float64, then f32 (lidars.py:327)
    ``elevations_deg`` + ``azimuth_steps`` n   ``phis = arange(-n / 2, n / 2) / (n / 2) pi`` in float64, then f32 (lidars.py:328)
    ``scan_csv``     path (relative to the file) of a Risley-prism scan table, see ``LidarSpec.from_scan_csv``.

The point cloud (``lidar_returns``, ``simulate_lidar_sweep``): ray r is a return iff ``acc[r] > acc_threshold`` (strict, f32, NaN
is not); the returns keep the ray order.  ``pts_world = o + d * range`` is one multiply then one add per component;
``pts_local = w2l pts_world`` sums every component in the fixed order ``((m0 x + m1 y) + m2 z) + t`` (the reference leaves the
order to its matmul).  The host reads ONE number per sweep, the return count, from host-mapped words without a stream
synchronisation.
"""
import bisect
import csv
import json
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib

MODES = {"grid": 0, "paired": 1}
_NOTIFY = None


def _f32(v) -> torch.Tensor:
    """angles as a host f32 vector; float64 input is rounded once, f32 tensors pass bit for bit"""
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().to(torch.float32).reshape(-1).contiguous()
    return torch.from_numpy(np.asarray(v, dtype=np.float64).astype(np.float32)).reshape(-1).contiguous()


class LidarSpec:
    """A sensor model: ``thetas``, ``phis`` (host f32), ``mode`` ("grid" | "paired"), ``axis`` (0 | 1), ``near``, ``far``, ``name``."""

    def __init__(self, thetas, phis, mode: str = "grid", axis: int = 0, near: float = 0.3, far: float = 120.0, name: str = "lidar",
                 rolling_shutter_effect: bool = False):
        if mode not in MODES:
            raise ValueError(f"lidar_sim: mode must be 'grid' or 'paired', got {mode!r}")
        if int(axis) not in (0, 1):
            raise ValueError(f"lidar_sim: axis must be 0 or 1, got {axis!r}")
        self.thetas, self.phis = _f32(thetas), _f32(phis)
        if mode == "paired" and self.thetas.numel() != self.phis.numel():
            raise ValueError(f"lidar_sim: a paired sensor takes as many thetas as phis, got {self.thetas.numel()} and "
                             f"{self.phis.numel()}")
        self.mode, self.axis, self.near, self.far, self.name = mode, int(axis), float(near), float(far), str(name)
        self.rolling_shutter_effect = bool(rolling_shutter_effect)
        self.slices: Optional[List[Tuple[torch.Tensor, torch.Tensor]]] = None     # scan tables: one paired slice per second
        self.cycle = 0

    @classmethod
    def spinning(cls, elevations_deg, azimuths_rad, near: float = 0.3, far: float = 120.0, axis: int = 0, name: str = "spinning"):
        """beam elevations in degrees above the horizon -> ``thetas = pi / 2 - elev pi / 180`` in float64 (lidars.py:327)"""
        elev = np.asarray(elevations_deg, dtype=np.float64)
        return cls(np.pi / 2.0 - elev / 180.0 * np.pi, azimuths_rad, "grid", axis, near, far, name)

    @classmethod
    def paired(cls, thetas, phis, near: float = 0.3, far: float = 120.0, axis: int = 0, name: str = "paired"):
        return cls(thetas, phis, "paired", axis, near, far, name)

    @classmethod
    def from_scan_csv(cls, path, near: float = 0.3, far: float = 90.0, name: Optional[str] = None):
        """A Risley-prism scan table (lidars.py:542-588): rows ``time, phi_deg, theta_deg`` with times ascending; angles are
        ``deg pi / 180`` (no ``pi / 2 -``).  With ``max_sec = int(max(time))`` the rows are cut into one paired slice per whole
        second, slice k = rows ``bisect_right(times, k) .. bisect_right(times, k + 1)`` (the first starts at row 0; rows after
        second ``max_sec`` are dropped); ``Lidar.get_all_rays`` fires slice ``cycle % max_sec`` and advances ``cycle``."""
        times, thetas, phis = [], [], []
        with open(path, mode="r", encoding="utf-8") as f:
            for row in csv.reader(f):
                if not row:
                    continue
                times.append(float(row[0]))
                phis.append(float(row[1]))
                thetas.append(float(row[2]))
        max_sec = max((int(t) for t in times), default=0)
        if max_sec < 1:
            raise ValueError(f"lidar_sim: {path} holds no whole second of scan rows")
        th = np.asarray(thetas, dtype=np.float64) / 180.0 * np.pi
        ph = np.asarray(phis, dtype=np.float64) / 180.0 * np.pi
        spec = cls(th, ph, "paired", 0, near, far, name if name is not None else Path(path).stem)
        spec.slices, pre = [], 0
        for sec in range(1, max_sec + 1):
            idx = bisect.bisect_right(times, sec)
            spec.slices.append((_f32(th[pre:idx]), _f32(ph[pre:idx])))
            pre = idx
        return spec

    @property
    def n_slices(self) -> int:
        return len(self.slices) if self.slices is not None else 1

    def take_slice(self) -> int:
        """index of the angle set the next sweep fires (0 for everything but scan tables, which cycle)"""
        if self.slices is None:
            return 0
        k = self.cycle % len(self.slices)
        self.cycle += 1
        return k

    def angles(self, k: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        return (self.thetas, self.phis) if self.slices is None else self.slices[k]


def load_sensor_specs(file) -> Dict[Tuple[str, str], LidarSpec]:
    """Sensor-description file (schema in the module docstring; a loaded object is taken as well) -> {(lidar_model, lidar_name):
    LidarSpec}."""
    base = Path(".")
    if isinstance(file, (str, Path)):
        base = Path(file).parent
        if str(file).endswith(".json"):
            with open(file, "r", encoding="utf-8") as f:
                obj = json.load(f)
        else:
            obj = torch.load(file, map_location="cpu", weights_only=True)
    else:
        obj = file
    entries = obj["sensors"] if isinstance(obj, dict) else obj
    out = {}
    for e in entries:
        key = (str(e["lidar_model"]), str(e["lidar_name"]))
        near, far = float(e.get("near", 0.3)), float(e.get("far", 120.0))
        if "scan_csv" in e:
            spec = LidarSpec.from_scan_csv(base / e["scan_csv"], near, far, name=key[1])
        else:
            if "thetas" in e:
                thetas = e["thetas"]
            else:
                thetas = np.pi / 2.0 - np.asarray(e["elevations_deg"], dtype=np.float64) / 180.0 * np.pi
            if "phis" in e:
                phis = e["phis"]
            else:
                n = int(e["azimuth_steps"])
                if n < 2 or n % 2:
                    raise ValueError(f"lidar_sim: azimuth_steps must be even and >= 2, got {n} for {key}")
                phis = np.arange(-(n // 2), n // 2, 1) / (n // 2) * np.pi
            spec = LidarSpec(thetas, phis, e.get("mode", "grid"), int(e.get("axis", 0)), near, far, key[1])
        spec.rolling_shutter_effect = bool(e.get("rolling_shutter_effect", False))
        out[key] = spec
    return out


def carla_to_opencv() -> torch.Tensor:
    """lidars.py:188-192"""
    m = torch.eye(4, dtype=torch.float32)
    m[:3, :3] = torch.tensor([[0.0, 1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    return m


def lidar_raygen(thetas: torch.Tensor, phis: torch.Tensor, l2w: torch.Tensor, mode: str = "grid", axis: int = 0,
                 return_theta_phi: bool = False):
    """``nsim_lidar_raygen`` on device tensors: thetas, phis f32 vectors, l2w f32 [3,4] (or [4,4]: its first three rows),
    contiguous -> rays_o [N,3], rays_d [N,3](, theta_phi [N,2])."""
    for t, n in ((thetas, "thetas"), (phis, "phis"), (l2w, "l2w")):
        _lib.require_device(t, n)
    if mode not in MODES:
        raise ValueError(f"lidar_sim: mode must be 'grid' or 'paired', got {mode!r}")
    if tuple(l2w.shape) not in ((3, 4), (4, 4)):
        raise ValueError(f"lidar_sim: l2w must be [3,4] or [4,4], got {tuple(l2w.shape)}")
    if not l2w.is_contiguous():
        raise ValueError("lidar_sim: l2w must be contiguous")
    if thetas.dim() != 1 or phis.dim() != 1:
        raise ValueError("lidar_sim: thetas and phis are vectors")
    nb, na = int(thetas.shape[0]), int(phis.shape[0])
    if mode == "paired" and nb != na:
        raise ValueError(f"lidar_sim: a paired sensor takes as many thetas as phis, got {nb} and {na}")
    N = nb * na if mode == "grid" else nb
    dev = l2w.device
    rays_o = torch.empty([N, 3], dtype=torch.float32, device=dev)
    rays_d = torch.empty([N, 3], dtype=torch.float32, device=dev)
    tp = torch.empty([N, 2], dtype=torch.float32, device=dev) if return_theta_phi else None
    _lib.call("nsim_lidar_raygen", _lib.ptr(thetas, torch.float32, "thetas"), _lib.ptr(phis, torch.float32, "phis"), nb, na,
              MODES[mode], int(axis), _lib.ptr(l2w, torch.float32, "l2w"), _lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(tp))
    return (rays_o, rays_d, tp) if return_theta_phi else (rays_o, rays_d)


class Lidar:
    """The ``Lidar`` node's surface (lidars.py:177-264) for one ``LidarSpec``: ``.near``, ``.far``, ``get_all_rays``."""

    def __init__(self, spec: LidarSpec, device=None):
        self.spec = spec
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.near, self.far = spec.near, spec.far
        self.rolling_shutter_effect = spec.rolling_shutter_effect
        self._dev_angles = {}
        self.last_shape = None

    @property
    def mode(self) -> str:
        return self.spec.mode

    def _angles(self, k: int):
        if k not in self._dev_angles:
            th, ph = self.spec.angles(k)
            self._dev_angles[k] = (th.to(self.device), ph.to(self.device))
        return self._dev_angles[k]

    def get_all_rays(self, l2w: torch.Tensor = None, *, world_transform: torch.Tensor = None, return_theta_phi: bool = False,
                     return_ts: bool = False, ts=None) -> List[torch.Tensor]:
        """-> [rays_o [N,3], rays_d [N,3](, theta_phi)(, rays_ts [N])] in the world.  ``l2w`` (device f32 [3,4] / [4,4],
        contiguous) is taken as is; ``world_transform`` [4,4] (the node's pose, host or device) is multiplied by the carla ->
        OpenCV matrix on the host first (lidars.py:211).  ``theta_phi`` is [n_az, n_beams, 2] for a grid sensor, [N, 2] for a
        paired one, as the reference's.  ``return_ts`` appends a tensor filled with ``ts`` (the frozen frame's time stamp or
        index); per-beam rolling-shutter time stamps are not implemented (lidars.py:259-262)."""
        if (l2w is None) == (world_transform is None):
            raise ValueError("lidar_sim: give exactly one of l2w and world_transform")
        if return_ts and self.rolling_shutter_effect:
            raise NotImplementedError("lidar_sim: per-beam time stamps under `rolling_shutter_effect` are not implemented "
                                      "(as in the reference, lidars.py:259-262)")
        if world_transform is not None:
            wt = torch.as_tensor(world_transform).detach().to(torch.float32).cpu()
            if tuple(wt.shape) != (4, 4):
                raise ValueError(f"lidar_sim: world_transform must be [4,4], got {tuple(wt.shape)}")
            l2w = (wt.unsqueeze(-1) * carla_to_opencv().unsqueeze(-3)).sum(-2)[:3].contiguous().to(self.device)
        thetas, phis = self._angles(self.spec.take_slice())
        out = list(lidar_raygen(thetas, phis, l2w, self.spec.mode, self.spec.axis, return_theta_phi))
        self.last_shape = (int(phis.shape[0]), int(thetas.shape[0])) if self.spec.mode == "grid" else (int(thetas.shape[0]),)
        if return_theta_phi and self.spec.mode == "grid":
            out[2] = out[2].view(phis.shape[0], thetas.shape[0], 2)
        if return_ts:
            n = out[0].shape[0]
            if ts is None:
                ts = 0
            if isinstance(ts, torch.Tensor):
                out.append(ts.to(out[0].device).reshape(-1)[:1].expand(n).contiguous())
            else:
                out.append(torch.full([n], ts, dtype=torch.float32 if isinstance(ts, float) else torch.long, device=out[0].device))
        return out


def _notify():
    global _NOTIFY
    if _NOTIFY is None:
        _NOTIFY = _lib.HostNotify(1)
    return _NOTIFY or None


def lidar_returns(acc: torch.Tensor, depth: torch.Tensor, rays_o: torch.Tensor, rays_d: torch.Tensor, *, w2l: torch.Tensor = None,
                  rgb: torch.Tensor = None, ids: torch.Tensor = None, acc_threshold: float = 0.95,
                  with_range_image: bool = False) -> Dict:
    """The stable compaction of a rendered sweep (render.py:331-346): acc, depth f32 [N], rays f32 [N,3], optional w2l f32 [3,4]
    (or [4,4]), rgb f32 [N,3], ids int64 [N] -> dict(rays_inds int64 [M], ranges, mask [M], pts_world [M,3], n_returns = M,
    [pts_local [M,3]], [rgb [M,3]], [ins_seg int64 [M]], [range_image [N]]), returns in ray order."""
    global _NOTIFY
    for t, n in ((acc, "acc"), (depth, "depth"), (rays_o, "rays_o"), (rays_d, "rays_d")):
        _lib.require_device(t, n)
    N, dev = int(acc.shape[0]), acc.device
    if acc.dim() != 1 or depth.shape != acc.shape or tuple(rays_o.shape) != (N, 3) or tuple(rays_d.shape) != (N, 3):
        raise ValueError("lidar_sim: acc, depth are [N] and rays_o, rays_d [N,3]")
    if w2l is not None:
        _lib.require_device(w2l, "w2l")
        if tuple(w2l.shape) not in ((3, 4), (4, 4)) or not w2l.is_contiguous():
            raise ValueError("lidar_sim: w2l must be a contiguous [3,4] or [4,4] tensor")
    if rgb is not None and tuple(rgb.shape) != (N, 3):
        raise ValueError("lidar_sim: rgb must be [N,3]")
    if ids is not None and tuple(ids.shape) != (N,):
        raise ValueError("lidar_sim: ids must be [N]")
    thr = float(acc_threshold)
    M = 0
    cnt = None
    if N > 0:
        nb = (N + 255) // 256
        cnt = torch.empty([nb], dtype=torch.int32, device=dev)
        tot = torch.empty([1], dtype=torch.int32, device=dev)
        _lib.call("nsim_lidar_returns_count", _lib.ptr(acc, torch.float32, "acc"), N, thr, _lib.ptr(cnt))
        nt = _notify()
        adr, seq = nt.arm(0) if nt is not None else (None, 0)
        _lib.call("nsim_occgrid_scan", _lib.ptr(cnt), nb, _lib.ptr(tot), adr, seq)
        M = nt.wait(0, seq) if nt is not None else None
        if M is None:                       # no host-mapped words, or the wait timed out: a synchronising read of the device copy
            M = int(tot.item())
            if nt is not None and int(nt.view[0, 1]) != seq:
                _NOTIFY = False             # finished and still not visible: this memory is not host-coherent
    f32 = dict(dtype=torch.float32, device=dev)
    out = dict(rays_inds=torch.empty([M], dtype=torch.long, device=dev), ranges=torch.empty([M], **f32),
               mask=torch.empty([M], **f32), pts_world=torch.empty([M, 3], **f32), n_returns=M)
    if w2l is not None:
        out["pts_local"] = torch.empty([M, 3], **f32)
    if rgb is not None:
        out["rgb"] = torch.empty([M, 3], **f32)
    if ids is not None:
        out["ins_seg"] = torch.empty([M], dtype=torch.long, device=dev)
    if with_range_image:
        out["range_image"] = torch.empty([N], **f32) if M > 0 else torch.zeros([N], **f32)
    if M > 0:
        _lib.call("nsim_lidar_returns_emit", _lib.ptr(acc), _lib.ptr(depth, torch.float32, "depth"),
                  _lib.ptr(rays_o, torch.float32, "rays_o"), _lib.ptr(rays_d, torch.float32, "rays_d"), N, thr, _lib.ptr(cnt),
                  _lib.ptr(w2l, torch.float32, "w2l"), _lib.ptr(rgb, torch.float32, "rgb"), _lib.ptr(ids, torch.long, "ids"),
                  _lib.ptr(out["rays_inds"]), _lib.ptr(out["ranges"]), _lib.ptr(out["mask"]), _lib.ptr(out["pts_world"]),
                  _lib.ptr(out.get("pts_local")), _lib.ptr(out.get("rgb")), _lib.ptr(out.get("ins_seg")),
                  _lib.ptr(out.get("range_image")))
    return out


def invert_pose(l2w: torch.Tensor) -> torch.Tensor:
    """world -> sensor matrix f32 [3,4] of a [3,4] / [4,4] pose, inverted in float64 on the host, on l2w's device"""
    m = torch.eye(4, dtype=torch.float64)
    m[:3] = l2w.detach().cpu().to(torch.float64)[:3]
    return torch.linalg.inv(m)[:3].to(torch.float32).contiguous().to(l2w.device)


@torch.no_grad()
def simulate_lidar_sweep(renderer, model_or_drawables, lidar: Lidar, l2w: torch.Tensor, *, forward_inv_s=None,
                         acc_threshold: float = 0.95, with_rgb: bool = False, with_segmentation: bool = False,
                         rayschunk: int = 65536, sky_model=None, distant_model=None, rays_h_appear: torch.Tensor = None,
                         w2l: torch.Tensor = None) -> Dict:
    """One sweep of ``lidar`` posed at ``l2w`` (device f32 [3,4] / [4,4]: sensor -> world, as ``get_all_rays`` takes it) through a
    trained scene, as render.py:319-346 does it: all rays, rendered in ``rayschunk`` pieces with the validation settings of
    ``eval.render_image`` (eval mode, ``perturb: false``, ``depth_use_normalized_vw: true``), close range only unless a sky /
    distant model is passed, ``with_normal=False``, ``near`` / ``far`` of the lidar, ``forward_inv_s`` passed to the models'
    ray query as the tools do; then ONE compaction over the whole sweep.
    ``model_or_drawables``: a model (``SingleVolumeRenderer.render``) or a list of ``Drawable`` (``BufferComposeRenderer.ray_query``,
    as ``eval.render_scene_image``).  ``w2l``: world -> local matrix of ``pts_local`` (default: the inverse of ``l2w``).
    -> dict(pts_world, pts_local [M,3], ranges, mask [M], rays_inds int64 [M], n_returns, range_image ([n_az, n_beams] for a grid
    sensor, else [N]), [rgb [M,3]], [ins_seg int64 [M]] (``ins_seg_mask_buffer`` at the returns), rays_o, rays_d).  Every
    output is per ray: the chunk size changes none of them."""
    rays_o, rays_d = lidar.get_all_rays(l2w)
    shape = lidar.last_shape
    N = rays_o.shape[0]
    compose = isinstance(model_or_drawables, (list, tuple))
    if with_segmentation and not compose:
        raise ValueError("lidar_sim: with_segmentation needs a drawable list (BufferComposeRenderer)")
    bypass = {"forward_inv_s": forward_inv_s} if forward_inv_s is not None else None
    ha = rays_h_appear.reshape(1, -1).expand(N, -1).contiguous() if rays_h_appear is not None else None
    step = int(rayschunk) if rayschunk and int(rayschunk) > 0 else max(N, 1)
    was_training, cfg_saved = renderer.training, dict(renderer.config)
    renderer.eval()
    renderer.config.update(perturb=False, depth_use_normalized_vw=True)
    acc, depth, rgb, ids = [], [], [], []

    def take(ret):
        r = ret["rendered"]
        acc.append(r["mask_volume"])
        depth.append(r["depth_volume"])
        if with_rgb:
            rgb.append(r["rgb_volume"])
        if with_segmentation:
            ids.append(ret["ins_seg_mask_buffer"])
    try:
        if compose:
            by = None
            if bypass is not None:
                by = {dr.class_name: bypass for dr in model_or_drawables}
                if distant_model is not None:
                    by["Distant"] = bypass
            for s in range(0, N, step):
                h = ha[s:s + step].contiguous() if ha is not None else None
                take(renderer.ray_query(rays_o[s:s + step].contiguous(), rays_d[s:s + step].contiguous(),
                                        drawables=list(model_or_drawables), rays_h_appear=h, near=lidar.near, far=lidar.far,
                                        with_rgb=with_rgb, with_normal=False, sky_model=sky_model, distant_model=distant_model,
                                        render_per_obj_individual=bool(with_segmentation), bypass_ray_query_cfg=by))
        elif N > 0:
            take(renderer.render(model_or_drawables, rays=[rays_o, rays_d], rays_h_appear=ha, near=lidar.near, far=lidar.far,
                                 rayschunk=step, with_rgb=with_rgb, with_normal=False, sky_model=sky_model,
                                 distant_model=distant_model, with_env=(sky_model is not None or distant_model is not None),
                                 bypass_ray_query_cfg=bypass))
    finally:
        renderer.train(was_training)
        renderer.config.clear()
        renderer.config.update(cfg_saved)

    def whole(vs, tail=(), dtype=torch.float32):
        if not vs:
            return torch.zeros([0, *tail], dtype=dtype, device=rays_o.device)
        return (torch.cat(vs) if len(vs) > 1 else vs[0]).to(dtype).contiguous()
    out = lidar_returns(whole(acc), whole(depth), rays_o, rays_d, w2l=w2l if w2l is not None else invert_pose(l2w),
                        rgb=whole(rgb, (3,)) if with_rgb else None, ids=whole(ids, (), torch.long) if with_segmentation else None,
                        acc_threshold=acc_threshold, with_range_image=True)
    if len(shape) == 2:
        out["range_image"] = out["range_image"].view(*shape)
    out.update(rays_o=rays_o, rays_d=rays_d)
    return out


def save_pcl_npy(path, ret: Dict):
    """The per-frame array of render.py:348-355: local xyz followed by rgb when rgb was rendered, otherwise by the mask."""
    cols = [ret["pts_local"], ret["rgb"] if "rgb" in ret else ret["mask"].unsqueeze(-1)]
    np.save(path, torch.cat(cols, dim=-1).contiguous().cpu().numpy())
