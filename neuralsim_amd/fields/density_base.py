"""What the marched density models share: ``MarchedDensityModel``, the base of ``LoTDNeRFModel`` (fields/nerf.py) and
``EmerNeRFOnlyDynamicModel`` (fields/dynamic_nerf.py) -- the ``march_occ`` ray query, the trainer hooks, the decoder parameters and
the occupancy accelerator's construction -- and the pieces their autograd backwards (and the distant models') have in common.
"""
from contextlib import contextmanager
from typing import Dict

import torch
import torch.nn as nn

from .. import _lib
from ..graphics import pack_ops as po
from ..model_base import ModelMixin
from ..spatial import cached_aabb_space
from .neus import _QueryCfg, rays_has_grad, volume_integration


def f32c(g):
    """An incoming gradient as the kernels read it (None stays None: that output had no consumer)."""
    return g.float().contiguous() if g is not None else None


def zero_grads_like(*params):
    """Zero-filled f32 gradient buffers of the flat parameters ``params``: one allocation (one fill), split."""
    sizes = [p.numel() for p in params]
    return _lib.zeros([sum(sizes)], device=params[0].device).split(sizes)


def reduce_ray_grads(dx, dv, t, ridx, ray_shape, need_x, need_o, need_d):
    """per-sample dx [S,3] (and dv) -> (d_x, d_o, d_d): dx itself for points, else the per-ray sums of
    ``nsim_ray_grad_reduce`` into zero-filled rows (a ray without samples gets an exact zero row)"""
    if need_x:
        return dx, None, None
    d_o = torch.zeros(list(ray_shape), dtype=torch.float32, device=dx.device) if need_o else None
    d_d = torch.zeros(list(ray_shape), dtype=torch.float32, device=dx.device) if need_d else None
    _lib.call("nsim_ray_grad_reduce", _lib.ptr(dx), _lib.ptr(dv), _lib.ptr(t), _lib.ptr(ridx), dx.shape[0], _lib.ptr(d_o),
              _lib.ptr(d_d))
    return None, d_o, d_d


class MarchedDensityModel(ModelMixin, nn.Module):
    """A subclass builds ``encoding``, ``meta``, the decoders (``_make_decoder``) and ``accel`` (``_make_accel``), names the yaml
    block of its appearance width in ``_appear_cfg`` and provides the hooks of ``ray_query``: ``_check_rays``, ``_march_extras``,
    ``_decode``, ``_collect`` -- and ``_set_active_raw`` behind ``_level_mask``."""
    is_ray_query_supported = True
    _appear_cfg = None

    @property
    def ray_query_cfg(self):
        return self._ray_query_cfg

    @ray_query_cfg.setter
    def ray_query_cfg(self, cfg):
        object.__setattr__(self, "_ray_query_cfg", _QueryCfg(cfg or {}))

    # ------------------------------------------------------------------ construction
    def _make_decoder(self, name: str, layers, g: torch.Generator):
        """``<name>_w`` / ``<name>_b``: the flat weights and biases of the linear ``layers`` [(out, in), ...], torch.nn.Linear's
        default init drawn from ``g`` layer by layer.  The backwards size their gradient buffers from these parameters."""
        ws, bs = [], []
        for o, i in layers:
            b = 1.0 / (i ** 0.5)
            ws.append(((torch.rand(o, i, generator=g) * 2 - 1) * b).reshape(-1))
            bs.append((torch.rand(o, generator=g) * 2 - 1) * b)
        setattr(self, name + "_w", nn.Parameter(torch.cat(ws)))
        setattr(self, name + "_b", nn.Parameter(torch.cat(bs)))

    def _make_accel(self, cls, *lead, acc: dict, resolution):
        """``self.accel = cls(*lead, ...)`` from the yaml's ``accel_cfg`` block ``acc``, initialised."""
        ufn = acc.get("update_from_net_cfg") or {}
        self.accel = cls(
            *lead, resolution=resolution, occ_thre=float(acc.get("occ_thre", 0.01)),
            ema_decay=float(acc.get("ema_decay", 0.95)), num_steps=int(ufn.get("num_steps", 4)),
            num_pts=int(ufn.get("num_pts", 2 ** 20)), n_steps_between_update=int(acc.get("n_steps_between_update", 16)),
            n_steps_warmup=int(acc.get("n_steps_warmup", 256)), update_from_samples_cfg=acc.get("update_from_samples_cfg", None),
            init_cfg=acc.get("init_cfg"), occ_thre_consider_mean=bool(acc.get("occ_thre_consider_mean", False)),
            constant_value=float((acc.get("init_cfg") or {}).get("constant_value", 1.0)))
        self.accel.init()

    # ------------------------------------------------------------------ reference life cycle
    def training_before_per_step(self, it: int, logger=None):
        """The occupancy refresh on the ``n_steps_*`` schedule, arming of the sample collection."""
        if self.accel.update_from_samples_cfg is not None:
            self.accel.collect_armed = True
        self.accel.cur_batch__step(int(it), self.query_density, generator=getattr(self, "refresh_generator", None))

    def training_after_per_step(self, it: int, logger=None):
        pass

    def model_setup(self):
        self._shadow()

    @property
    def device(self):
        return self.den_w.device

    @property
    def space(self):
        return cached_aabb_space(self, self.accel.aabb)

    # ------------------------------------------------------------------ kernels' inputs
    def _active_levels(self) -> int:
        return int(self.meta.lotd.n_active_levels)

    @contextmanager
    def _level_mask(self, n: int):
        """The backward of a query uses the level mask the query was made with, whatever has been set since."""
        prev = self._active_levels()
        self._set_active_raw(n)
        try:
            yield
        finally:
            self._set_active_raw(prev)

    def _step(self, cfg: dict = None) -> float:
        qp = (cfg or {}).get("query_param", None) or self.ray_query_cfg.get("query_param", {})
        return float((qp.get("march_cfg") or {}).get("step_size", 0.1))

    # ------------------------------------------------------------------ rays
    def _check_rays(self, ray_tested: dict, has_grad: bool):
        """Raise on per-ray inputs that are missing or require a gradient the model does not build."""
        raise NotImplementedError

    def _march_extras(self, ray_tested: dict):
        """-> (the marcher's per-ray word offset into the occupancy bits | None, per-ray inputs of ``_decode`` | None, extra
        ``details`` entries)."""
        return None, None, {}

    def _decode(self, ray_tested, h_appear, o, d, t, ridx, w, step, with_rgb):
        """-> (sigma [S], alpha [S], rgb [S,3] | None, extra volume-buffer entries) at the samples o[ridx] + t d[ridx]."""
        raise NotImplementedError

    def _collect(self, sigma, rays, extras: dict):
        """``accel.collect`` of the step's own samples; ``extras``: what ``_march_extras`` returned last."""
        raise NotImplementedError

    def ray_query(self, *, ray_input: dict = None, ray_tested: dict, config=None, return_buffer: bool = True,
                  return_details: bool = False, render_per_obj_individual: bool = False, with_rgb: bool = None,
                  with_normal: bool = None, **unused) -> Dict:
        """``query_mode: march_occ``: the samples are the marcher's lattice t_k = near + (k + jitter) step inside occupied
        voxels (of the slice of each ray's time, for a time-sliced accelerator; jitter per ray when ``perturb``, else 0); every
        sample's interval is ``step``."""
        cfg = dict(config or {})
        mode = cfg.get("query_mode", self.ray_query_cfg.get("query_mode", "march_occ"))
        if mode != "march_occ":
            raise NotImplementedError(f"ray_query_cfg.query_mode={mode!r}: march_occ is built")
        if cfg.get("with_feature_dim", 0):
            raise NotImplementedError("with_feature_dim > 0: the decoders of this model emit no extra feature channels")
        with_rgb = cfg.get("with_rgb", True) if with_rgb is None else bool(with_rgb)
        qp = dict(cfg.get("query_param", None) or self.ray_query_cfg.get("query_param", {}))
        march = qp.get("march_cfg") or {}
        step, max_steps = float(march.get("step_size", 0.1)), int(march.get("max_steps", 4096))
        n_all = None
        if render_per_obj_individual and ray_input is not None and ray_input.get("rays_o") is not None:
            n_all = int(ray_input["rays_o"].shape[0])

        def empty(details=None):
            ret = dict(volume_buffer=dict(type="empty"))
            if render_per_obj_individual:
                dev_ = ray_tested["rays_inds"].device
                z = lambda *sh: torch.zeros([n_all or 0, *sh], dtype=torch.float32, device=dev_)      # noqa: E731
                ret["rendered"] = dict(mask_volume=z(), depth_volume=z())
                if with_rgb:
                    ret["rendered"]["rgb_volume"] = z(3)
            if return_details:
                ret["details"] = details or {}
            return ret
        R = int(ray_tested["num_rays"])
        if R == 0:
            return empty()
        self._check_rays(ray_tested, rays_has_grad(self.ray_query_cfg, cfg))
        # marching, the occupancy grid and the sample depths see detached rays; the decoders' samples o + t d carry the graph
        o = ray_tested["rays_o"].detach().float().contiguous()
        d = ray_tested["rays_d"].detach().float().contiguous()
        near, far = ray_tested["near"].detach().float().contiguous(), ray_tested["far"].detach().float().contiguous()
        dev = o.device
        jitter = cfg.get("_jitter", None)
        if jitter is None:
            jitter = torch.rand([R], device=dev) if cfg.get("perturb", False) else torch.zeros([R], device=dev)
        jitter = jitter.float().contiguous()
        acc = self.accel
        bits, occm = acc.occ_bits, acc.meta
        with torch.no_grad():
            woff, w, extras = self._march_extras(ray_tested)
            counts = torch.empty([R], dtype=torch.long, device=dev)
            _lib.call("nsim_march_count", _lib.ptr(o), _lib.ptr(d), _lib.ptr(near), _lib.ptr(far), _lib.ptr(jitter), R,
                      _lib.ptr(bits), _lib.ptr(woff), occm, step, max_steps, _lib.ptr(counts))
            pi, total = po.get_pack_infos_from_n(counts, return_total=True)
            S = int(total.item())                    # host sync: size of the marched set
            if S == 0:
                acc.collect_armed = False
                return empty(dict(march_counts=counts, **extras))
            t = torch.empty([S], dtype=torch.float32, device=dev)
            _lib.call("nsim_march_emit", _lib.ptr(o), _lib.ptr(d), _lib.ptr(near), _lib.ptr(far), _lib.ptr(jitter), R,
                      _lib.ptr(bits), _lib.ptr(woff), occm, step, max_steps, _lib.ptr(pi), _lib.ptr(t))
            ridx = torch.repeat_interleave(torch.arange(R, device=dev), counts, output_size=S)
            sel = counts.nonzero()[:, 0]
        h_appear = ray_tested.get("rays_h_appear", None) if (with_rgb and self.n_appear) else None
        if with_rgb and self.n_appear and h_appear is None:
            raise ValueError(f"ray_tested['rays_h_appear'] is missing: {self._appear_cfg}.n_appear_embedding is "
                             f"{self.n_appear}, the radiance decoder reads a per-ray appearance code")
        sigma, alpha, rgb, vb_extra = self._decode(ray_tested, h_appear, o, d, t, ridx, w, step, bool(with_rgb))
        if acc.collect_armed:
            self._collect(sigma, (o, d, t, ridx), extras)
            acc.collect_armed = False
        vb = dict(type="packed", rays_inds_hit=ray_tested["rays_inds"][sel], pack_infos_hit=pi[sel], t=t, sigma=sigma,
                  opacity_alpha=alpha)
        if with_rgb:
            vb["rgb"] = rgb
        vb.update(vb_extra)
        ret = dict(volume_buffer=vb)
        if render_per_obj_individual or cfg.get("_render", False):
            ret["rendered"] = volume_integration(alpha, t, rgb if with_rgb else None, None, pi,
                                                 cfg.get("depth_use_normalized_vw", True),
                                                 rays_inds=ray_tested["rays_inds"] if n_all is not None else None, num_rays=n_all)
            ret["rendered"].pop("vw", None)
            ret["rendered"].pop("trans", None)
        if return_details:
            ret["details"] = dict(march_counts=counts, ridx=ridx, pack_infos=pi, **extras)
        return ret
