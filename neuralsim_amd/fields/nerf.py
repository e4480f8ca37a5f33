"""Close-range LoTD NeRF model (InstantNGP + UrbanNeRF) -- host side of csrc/nerf_field.hip's ``k_ngp`` kernels.

Mirrors ``nr3d_lib.models.fields.nerf.LoTDNeRFModel`` as the reference wraps and drives it (``LoTDNeRFObj`` /
``LoTDNeRFStreet``, app/models/single/nerf.py:33-143; docs/methods/ngp_lidar.md; config
code_single/configs/waymo/ngp_withlidar.230814.yaml:100-167).  The implementation lives in the absent nr3d_lib: the
semantics are this package's reading of the yaml, recorded in DESIGN.md sec. 7; tests/nerf_ref.py is the executable spec.

All arithmetic runs in HIP kernels: the 3-D LoTD gather / scatter of csrc/field.hip, the occupancy marcher of
csrc/sampling.hip, and the fused density + radiance decoders, their backward and the density occupancy folds of
csrc/nerf_field.hip.  This file allocates tensors, sequences launches and defines the autograd boundary.
"""
from typing import Dict, Optional

import torch

from .. import _lib
from ..grid_encodings.lotd import LoTDConfig, LoTDEncoding
from ..spatial import aabb_ray_test
from .density_base import MarchedDensityModel, f32c, reduce_ray_grads, zero_grads_like
from .neus import OccGridAccel


class DensityOccGridAccel(OccGridAccel):
    """``accel_cfg{type: occ_grid, resolution, occ_thre, occ_thre_consider_mean, ema_decay, init_cfg{mode: constant,
    constant_value}, update_from_net_cfg, update_from_samples_cfg: {}, n_steps_between_update, n_steps_warmup}`` of a
    density field (ngp_withlidar.230814.yaml:138-152).  There is no ``occ_val_fn_cfg``: the value grid holds densities.
    A voxel is occupied when ``val > thre``, ``thre = min(occ_thre, mean(val))`` with ``occ_thre_consider_mean`` -- the mean
    is taken on the device (``nsim_occ_pack_bits_mean``), the threshold used is kept in ``occ_thre_dev``."""

    def __init__(self, aabb, occ_thre_consider_mean: bool = False, constant_value: float = 1.0, **kw):
        dev = kw.pop("device", None)
        super().__init__(aabb, **kw)
        self.occ_thre_consider_mean = bool(occ_thre_consider_mean)
        self.constant_value = float(constant_value)
        self.register_buffer("occ_thre_dev", torch.full([1], self.occ_thre, dtype=torch.float32))
        self.register_buffer("_mean_ws", torch.zeros([65], dtype=torch.float32), persistent=False)
        if dev is not None:
            self.to(dev)

    def _occupied(self) -> torch.Tensor:
        """bool [n_voxels] in storage order: the bits the marcher reads (``init`` marks every voxel whatever its value)."""
        sh = torch.arange(32, dtype=torch.int32, device=self.occ_bits.device)
        return ((self.occ_bits.view(-1, 1) >> sh) & 1).bool().reshape(-1)[:self.occ_val.shape[0]]

    @property
    def occ_grid(self) -> torch.Tensor:
        r = self.resolution
        return self._occupied().view(r[2], r[1], r[0]).permute(2, 1, 0)

    def frac_occupied(self) -> float:
        return float(self._occupied().float().mean())

    def set_all_occupied(self):
        self.occ_val.fill_(max(self.constant_value, 2.0 * self.occ_thre, 1e-30))
        self.pack_bits()

    def pack_bits(self):
        _lib.call("nsim_occ_pack_bits_mean", _lib.ptr(self.occ_val), self.occ_val.shape[0], self.occ_thre,
                  int(self.occ_thre_consider_mean), _lib.ptr(self._mean_ws), _lib.ptr(self.occ_bits))
        self.occ_thre_dev = self._mean_ws[64:65].clone()

    @torch.no_grad()
    def update_from_samples(self, pts, sigma, pack=True):
        """val = max(val * ema_decay, sigma(p))."""
        pts = pts.detach().float().contiguous()
        sigma = sigma.detach().float().contiguous()
        _lib.call("nsim_occ_update_density", _lib.ptr(self.occ_val), self.occ_val.shape[0], self.ema_decay, _lib.ptr(pts),
                  _lib.ptr(sigma), pts.shape[0], self.meta)
        if pack:
            self.pack_bits()

    @torch.no_grad()
    def collect(self, pts=None, sigma=None, n_dev=None, n_add=0, rays=None):
        """Max-fold the densities of a training step's own samples (no decay, bits untouched): ``pts`` [n,3], or
        ``rays`` = (rays_o, rays_d, t, ridx)."""
        o, d, t, ridx = rays if rays is not None else (None, None, None, None)
        _lib.call("nsim_occ_collect_density", _lib.ptr(self.occ_val), _lib.ptr(pts), _lib.ptr(o), _lib.ptr(d), _lib.ptr(t),
                  _lib.ptr(ridx), _lib.ptr(sigma.detach().float().contiguous()), sigma.shape[0], self.meta)

    def init(self, query_density=None, logger=None, **kw):
        """``init_cfg{mode: constant, constant_value}``: every voxel holds the constant and is occupied."""
        self.occ_val.fill_(self.constant_value)
        self.occ_bits.fill_(-1)
        self.occ_thre_dev = torch.full_like(self.occ_thre_dev, min(self.occ_thre, self.constant_value)
                                            if self.occ_thre_consider_mean else self.occ_thre)
        # (all occupied whatever the threshold: a constant grid has val == mean, and ``val > mean`` would empty it)


class _NgpFn(torch.autograd.Function):
    """(table, den_w, den_b, rad_w, rad_b, h_appear) -> (sigma [S], alpha [S] [, rgb [S,3]]) at x [S,3] or at
    rays_o[ridx] + t rays_d[ridx]: level-major gather, then the fused decoders on the planes.  When x, or rays_o / rays_d,
    require grad (pose refinement; the model opts in with ``rays_has_grad``) the backward also returns their gradients:
    ``nsim_ngp_bwd_pose`` -> ``nsim_lotd_dx_lm`` -> ``nsim_ray_grad_reduce``; t is a constant of the step."""

    @staticmethod
    def forward(ctx, model, grid, den_w, den_b, rad_w, rad_b, h_appear, x, rays_o, rays_d, t, ridx, step, with_rgb):
        dev = grid.device
        S = x.shape[0] if x is not None else t.shape[0]
        grid16, wpack = model._shadow()
        need_bwd = any(ctx.needs_input_grad)
        PS = _lib.plane_pitch(S)
        h_pl = model._gather(grid16, x, rays_o, rays_d, t, ridx, S, dev)
        sigma = torch.empty([S], dtype=torch.float32, device=dev)
        alpha = torch.empty([S], dtype=torch.float32, device=dev)
        rgb = torch.empty([S, 3], dtype=torch.float32, device=dev) if with_rgb else None
        ha = h_appear.detach().float().contiguous() if (h_appear is not None and with_rgb and model.n_appear) else None
        _lib.call("nsim_ngp_fwd", model.meta, _lib.ptr(wpack), _lib.ptr(h_pl), PS, _lib.ptr(x), _lib.ptr(rays_o),
                  _lib.ptr(rays_d), _lib.ptr(t), _lib.ptr(ridx), _lib.ptr(ha), S, float(step), _lib.ptr(sigma),
                  _lib.ptr(alpha), _lib.ptr(rgb))
        if _lib.TIMER is not None:
            _lib.TIMER.note_units("nsim_ngp_fwd", S)
        ctx.model, ctx.S, ctx.PS, ctx.step, ctx.with_rgb = model, S, PS, float(step), with_rgb
        ctx.n_active = int(model.meta.lotd.n_active_levels)
        ctx.ha_shape = h_appear.shape if ha is not None else None
        ctx.set_materialize_grads(False)
        pose_in = any(ctx.needs_input_grad[7:10])       # (the table the forward read: the backward's nsim_lotd_dx_lm)
        ctx.save_for_backward(x, rays_o, rays_d, t, ridx, ha, h_pl if need_bwd else None, sigma, rgb, grid16 if pose_in else None)
        return (sigma, alpha, rgb) if with_rgb else (sigma, alpha)

    @staticmethod
    def backward(ctx, g_sigma, g_alpha, g_rgb=None):
        model = ctx.model
        x, rays_o, rays_d, t, ridx, ha, h_pl, sigma, rgb, grid16 = ctx.saved_tensors
        need = ctx.needs_input_grad
        n_out = 14
        if g_sigma is None and g_alpha is None and g_rgb is None:
            return (None,) * n_out
        dev, S = sigma.device, ctx.S
        wpack = model._shadow()[1]
        dden_w, dden_b, drad_w, drad_b = zero_grads_like(model.den_w, model.den_b, model.rad_w, model.rad_b)
        gs, ga, gr = f32c(g_sigma), f32c(g_alpha), f32c(g_rgb if ctx.with_rgb else None)
        dha = _lib.zeros(list(ctx.ha_shape), device=dev) if (ha is not None and need[6] and gr is not None) else None
        dgrid = _lib.zeros([model.encoding.cfg.n_params], device=dev) if need[1] else None
        need_x, need_o, need_d = need[7] and x is not None, need[8] and x is None, need[9] and x is None
        pose = need_x or need_o or need_d
        dh_pl = torch.empty([16, S, 2], dtype=torch.float32, device=dev) if (dgrid is not None or pose) else None
        dx = torch.empty([S, 3], dtype=torch.float32, device=dev) if pose else None
        dv = torch.empty([S, 3], dtype=torch.float32, device=dev) if (need_d and gr is not None) else None
        d_x = d_o = d_d = None
        meta = model.meta
        with model._level_mask(ctx.n_active):
            args = (meta, _lib.ptr(wpack), _lib.ptr(h_pl), ctx.PS, _lib.ptr(x), _lib.ptr(rays_o),
                    _lib.ptr(rays_d), _lib.ptr(t), _lib.ptr(ridx), _lib.ptr(ha), S, ctx.step, _lib.ptr(sigma.detach()),
                    _lib.ptr(rgb.detach()) if rgb is not None else None, _lib.ptr(gs), _lib.ptr(ga), _lib.ptr(gr),
                    _lib.ptr(dh_pl), _lib.ptr(dden_w), _lib.ptr(dden_b), _lib.ptr(drad_w), _lib.ptr(drad_b), _lib.ptr(dha))
            if pose:
                _lib.call("nsim_ngp_bwd_pose", *args, _lib.ptr(dx), _lib.ptr(dv))
                _lib.call("nsim_lotd_dx_lm", meta.lotd, _lib.ptr(grid16), _lib.ptr(x), _lib.ptr(rays_o),
                          _lib.ptr(rays_d), _lib.ptr(t), _lib.ptr(ridx), S, _lib.ptr(dh_pl), S, _lib.ptr(dx), _lib.ptr(dx))
                d_x, d_o, d_d = reduce_ray_grads(dx, dv, t, ridx, None if need_x else rays_o.shape, need_x, need_o, need_d)
            else:
                _lib.call("nsim_ngp_bwd", *args)
            if dgrid is not None:
                _lib.call("nsim_lotd_scatter", meta.lotd, _lib.ptr(x), _lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(t),
                          _lib.ptr(ridx), None, S, _lib.ptr(dh_pl), _lib.ptr(dh_pl), None, _lib.ptr(dgrid), 0, 0)
                # (the scatter reads a g plane next to dh whatever gn is; with gn == NULL it is multiplied by zero: dh stands in)
        if _lib.TIMER is not None:
            _lib.TIMER.note_units("nsim_ngp_bwd", S)
            if dgrid is not None:
                _lib.TIMER.note_units("nsim_lotd_scatter", S)
        if gr is None:      # no consumer of the colour: the radiance network is not part of the graph (None, not zeros)
            drad_w = drad_b = dha = None
        return (None, dgrid, dden_w, dden_b, drad_w, drad_b, dha, d_x, d_o, d_d) + (None,) * 4


class LoTDNeRFModel(MarchedDensityModel):
    _appear_cfg = "radiance_decoder_cfg"

    def __init__(self, aabb: torch.Tensor = None, seed: int = 42, device=None, **model_params):
        """``model_params``: the reference's yaml block verbatim (ngp_withlidar.230814.yaml:101-158; fields/ref_config.py
        ``validate_nerf_params`` names every option the kernels do not cover).  ``lotd_use_cuboid: true`` sizes the pyramid
        from the AABB: built by ``populate(aabb=...)`` (app/models/single/nerf.py:143)."""
        super().__init__()
        from . import ref_config
        self._params, self._seed = dict(model_params), int(seed)
        self._pending_device = device
        self.cfgd = ref_config.validate_nerf_params(self._params)
        self._built = False
        if aabb is not None or not self.cfgd["cuboid"]:
            if aabb is None:
                aabb = torch.tensor([[-1.0, -1, -1], [1.0, 1, 1]])
            self._build(torch.as_tensor(aabb, dtype=torch.float32).reshape(2, 3).cpu())
            if device is not None:
                self.to(device)

    def _build(self, aabb: torch.Tensor):
        from . import ref_config
        c = self.cfgd
        lod_res, log2_T = ref_config.nerf_lod_res(c, aabb)
        self.encoding = LoTDEncoding(LoTDConfig(lod_res, 2, log2_T), bound=c["param_bound"], seed=self._seed)
        self.encoding.cfg.set_aabb(aabb)
        assert self.encoding.cfg.num_levels <= 16
        F, NA = self.encoding.cfg.out_features, c["n_appear"]
        self.n_appear = NA
        g = torch.Generator().manual_seed(self._seed + 1)
        self._make_decoder("den", [(64, F + 3), (32, 64)], g)
        self._make_decoder("rad", [(64, 47 + NA), (64, 64), (3, 64)], g)
        acc = c["accel_cfg"]
        self._make_accel(DensityOccGridAccel, aabb, acc=acc, resolution=acc.get("resolution", (64, 64, 64)))
        self.ray_query_cfg = c["ray_query_cfg"]
        m = _lib.NgpMeta()
        m.lotd = self.encoding.cfg.meta
        m.precision = {"fp16": 0, "f32": 1}[c["precision"]]
        m.n_appear = NA
        self.meta = m
        fm32 = _lib.FieldMeta()         # the gather of csrc/field.hip reads the pyramid through a field meta (f32 planes)
        fm32.lotd, fm32.sdf_D, fm32.precision, fm32.softplus_beta, fm32.embed_E = m.lotd, 1, 1, 100.0, 0
        self._fm32 = fm32
        self._wpack, self._wpack_versions = None, None
        self._built = True
        self._sync_levels()

    # ------------------------------------------------------------------ reference life cycle
    def populate(self, aabb: torch.Tensor = None, device=None, **unused):
        """``populate(device=)`` (LoTDNeRFObj) / ``populate(aabb=, device=)`` (LoTDNeRFStreet: the cubic or cuboid box of
        ``populate_cfg.use_cuboid``, app/models/single/nerf.py:111-143)."""
        device = device if device is not None else self._pending_device
        if aabb is not None:
            a = torch.as_tensor(aabb, dtype=torch.float32).reshape(2, 3).cpu()
            if not self._built or not torch.equal(a, self.accel.aabb.cpu()):
                self._build(a)
        elif not self._built:
            raise AssertionError("lotd_use_cuboid sizes the pyramid from the AABB: populate(aabb=...)")
        if device is not None:
            self.to(device)
        return self

    @torch.no_grad()
    def training_initialize(self, config=None, logger=None, log_prefix=None) -> bool:
        """No pre-training: the occupancy grid's ``init`` (constant, all occupied) and the annealing state of iteration 0."""
        self.accel.init()
        self._anneal(0)
        return False

    def _param_groups(self, cfg: dict):
        enc = self.encoding
        enc.shadow()
        return [dict(name="encoding", params=[enc.flattened_params], shadow16=lambda: enc.shadow()),
                dict(name="density_decoder", params=[self.den_w, self.den_b]),
                dict(name="radiance_decoder", params=[self.rad_w, self.rad_b])]

    def _after_optimizer_step(self):
        self._wpack_versions = None

    def _weight_reg_tensors(self):
        return [self.den_w, self.rad_w]

    def set_active_levels(self, n: Optional[int]):
        self.encoding.cfg.set_active_levels(n)
        self._sync_levels()

    def _sync_levels(self):
        n = self.encoding.cfg.meta.n_active_levels
        self.meta.lotd.n_active_levels = n
        self._fm32.lotd.n_active_levels = n

    def _set_active_raw(self, n: int):
        self.meta.lotd.n_active_levels = n          # (the decoder launches' mask: all the backward reads)

    def _anneal(self, it: int):
        """``anneal_cfg{type: hardmask, start_level, start_it, stop_it}``, the NeuS model's rule (fields/neus.py
        ``anneal_levels``): level l is active once it >= start_it + (l - start_level) / (L - 1 - start_level) (stop_it - start_it)."""
        an = self.cfgd["anneal"]
        if an is None:
            return None
        L = self.encoding.cfg.num_levels
        r = min(max((it - an["start_it"]) / max(1, an["stop_it"] - an["start_it"]), 0.0), 1.0)
        n = int((an["start_level"] + r * (L - 1 - an["start_level"]) + 1e-9) // 1) + 1
        self.set_active_levels(max(n, 1))
        return n

    def training_before_per_step(self, it: int, logger=None):
        """Level annealing, the occupancy refresh on the ``n_steps_*`` schedule, arming of the sample collection."""
        self._anneal(int(it))
        super().training_before_per_step(it, logger)

    # ------------------------------------------------------------------ kernels' inputs
    def _shadow(self):
        """(fp16 table shadow, MFMA-fragment weight pack), refreshed lazily when a parameter changed in place."""
        grid16 = self.encoding.shadow()
        vers = (self.den_w._version, self.den_b._version, self.rad_w._version, self.rad_b._version, self.meta.precision,
                str(self.den_w.device), self.den_w.data_ptr())
        return grid16, self._weight_pack(
            "_wpack", vers, self.den_w.device, lambda: _lib.get_lib().nsim_ngp_wpack_bytes(self.meta),
            lambda buf: _lib.call("nsim_ngp_pack_weights", self.meta, _lib.ptr(self.den_w.detach()), _lib.ptr(self.den_b.detach()),
                                  _lib.ptr(self.rad_w.detach()), _lib.ptr(self.rad_b.detach()), _lib.ptr(buf)))

    def _gather(self, grid16, x, rays_o, rays_d, t, ridx, S, dev):
        """Level-major f32 feature planes [16][P][2] of S points (``nsim_lotd_gather_lm`` on the f32 meta: features only,
        no dh/dx planes -- the rays get no gradient); the backward reads the same planes."""
        h_pl = torch.empty([16, _lib.plane_pitch(S), 2], dtype=torch.float32, device=dev)
        _lib.call("nsim_lotd_gather_lm", self._fm32, _lib.ptr(grid16), _lib.ptr(x), _lib.ptr(rays_o), _lib.ptr(rays_d),
                  _lib.ptr(t), _lib.ptr(ridx), None, S, None, 0, _lib.ptr(h_pl))
        return h_pl

    # ------------------------------------------------------------------ point queries
    def forward_density(self, x: torch.Tensor, x_has_grad: bool = False) -> Dict[str, torch.Tensor]:
        """sigma at x [..., 3] (object coordinates), with gradient to the table and the density decoder -- and, with
        ``x_has_grad=True``, to x (pose refinement)."""
        if x.requires_grad and not x_has_grad:
            raise NotImplementedError("x.requires_grad: gradients to positions (pose refinement) are not built for this model "
                                      "unless asked for: forward_density(x, x_has_grad=True)")
        shape = x.shape[:-1]
        xf = x.float().reshape(-1, 3).contiguous() if (x_has_grad and x.requires_grad) else x.detach().float().reshape(-1, 3).contiguous()
        if xf.shape[0] == 0:
            return dict(sigma=torch.zeros(shape, dtype=torch.float32, device=xf.device))
        sigma, _ = _NgpFn.apply(self, self.encoding.flattened_params, self.den_w, self.den_b, self.rad_w, self.rad_b, None,
                                xf, None, None, None, None, self._step(), False)
        return dict(sigma=sigma.reshape(shape))

    @torch.no_grad()
    def query_density(self, x: torch.Tensor) -> torch.Tensor:
        return self.forward_density(x)["sigma"]

    def sample_pts_uniform(self, num_pts: int, generator=None) -> Dict[str, torch.Tensor]:
        """Random points of the AABB -> ``{'x', 'sigma'}`` with gradient (``SparsityLoss{type: density_reg, key: sigma}``)."""
        lo, hi = self.accel.aabb[0], self.accel.aabb[1]
        x = lo + torch.rand([num_pts, 3], device=self.device, generator=generator) * (hi - lo)
        ret = self.forward_density(x)
        ret["x"] = ret["net_x"] = x
        return ret

    # ------------------------------------------------------------------ rays
    def ray_test(self, rays_o, rays_d, near=None, far=None, **extra) -> Dict:
        return aabb_ray_test(self.accel.aabb, self.accel.meta, rays_o, rays_d, near=near, far=far, **extra)

    def _check_rays(self, ray_tested, has_grad):
        for k in ("rays_o", "rays_d"):
            if ray_tested[k].requires_grad and not has_grad:
                raise NotImplementedError(f"ray_tested[{k!r}].requires_grad: gradients to rays (pose refinement) are not built "
                                          f"for this model unless ray_query_cfg.query_param.rays_has_grad is set")

    def _decode(self, ray_tested, h_appear, o, d, t, ridx, w, step, with_rgb):
        ro, rd = ray_tested["rays_o"], ray_tested["rays_d"]
        outs = _NgpFn.apply(self, self.encoding.flattened_params, self.den_w, self.den_b, self.rad_w, self.rad_b, h_appear, None,
                            ro.float().contiguous() if ro.requires_grad else o, rd.float().contiguous() if rd.requires_grad else d,
                            t, ridx, step, with_rgb)
        return outs[0], outs[1], (outs[2] if with_rgb else None), {}

    def _collect(self, sigma, rays, extras):
        self.accel.collect(sigma=sigma, rays=rays)
