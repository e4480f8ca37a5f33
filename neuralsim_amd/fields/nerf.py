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
import torch.nn as nn

from .. import _lib
from ..graphics import pack_ops as po
from ..grid_encodings.lotd import LoTDConfig, LoTDEncoding
from ..model_base import ModelMixin
from ..spatial import aabb_ray_test
from .neus import OccGridAccel, _QueryCfg, rays_has_grad


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
        F, NA = model.encoding.cfg.out_features, model.n_appear
        n_dw, n_db, n_rw, n_rb = 64 * (F + 3) + 2048, 96, 64 * (47 + NA) + 4096 + 192, 131
        dden_w, dden_b, drad_w, drad_b = _lib.zeros([n_dw + n_db + n_rw + n_rb], device=dev).split([n_dw, n_db, n_rw, n_rb])
        gs = g_sigma.float().contiguous() if g_sigma is not None else None
        ga = g_alpha.float().contiguous() if g_alpha is not None else None
        gr = g_rgb.float().contiguous() if (ctx.with_rgb and g_rgb is not None) else None
        dha = _lib.zeros(list(ctx.ha_shape), device=dev) if (ha is not None and need[6] and gr is not None) else None
        dgrid = _lib.zeros([model.encoding.cfg.n_params], device=dev) if need[1] else None
        need_x, need_o, need_d = need[7] and x is not None, need[8] and x is None, need[9] and x is None
        pose = need_x or need_o or need_d
        dh_pl = torch.empty([16, S, 2], dtype=torch.float32, device=dev) if (dgrid is not None or pose) else None
        dx = torch.empty([S, 3], dtype=torch.float32, device=dev) if pose else None
        dv = torch.empty([S, 3], dtype=torch.float32, device=dev) if (need_d and gr is not None) else None
        d_x = d_o = d_d = None
        meta = model.meta
        prev = int(meta.lotd.n_active_levels)       # the backward of a query uses the level mask the query was made with
        meta.lotd.n_active_levels = ctx.n_active
        try:
            args = (meta, _lib.ptr(wpack), _lib.ptr(h_pl), ctx.PS, _lib.ptr(x), _lib.ptr(rays_o),
                    _lib.ptr(rays_d), _lib.ptr(t), _lib.ptr(ridx), _lib.ptr(ha), S, ctx.step, _lib.ptr(sigma.detach()),
                    _lib.ptr(rgb.detach()) if rgb is not None else None, _lib.ptr(gs), _lib.ptr(ga), _lib.ptr(gr),
                    _lib.ptr(dh_pl), _lib.ptr(dden_w), _lib.ptr(dden_b), _lib.ptr(drad_w), _lib.ptr(drad_b), _lib.ptr(dha))
            if pose:
                _lib.call("nsim_ngp_bwd_pose", *args, _lib.ptr(dx), _lib.ptr(dv))
                _lib.call("nsim_lotd_dx_lm", meta.lotd, _lib.ptr(grid16), _lib.ptr(x), _lib.ptr(rays_o),
                          _lib.ptr(rays_d), _lib.ptr(t), _lib.ptr(ridx), S, _lib.ptr(dh_pl), S, _lib.ptr(dx), _lib.ptr(dx))
                if need_x:
                    d_x = dx
                else:       # (zero-filled: a ray without samples gets an exact zero row)
                    d_o = torch.zeros_like(rays_o) if need_o else None
                    d_d = torch.zeros_like(rays_d) if need_d else None
                    _lib.call("nsim_ray_grad_reduce", _lib.ptr(dx), _lib.ptr(dv), _lib.ptr(t), _lib.ptr(ridx), S,
                              _lib.ptr(d_o), _lib.ptr(d_d))
            else:
                _lib.call("nsim_ngp_bwd", *args)
            if dgrid is not None:
                _lib.call("nsim_lotd_scatter", meta.lotd, _lib.ptr(x), _lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(t),
                          _lib.ptr(ridx), None, S, _lib.ptr(dh_pl), _lib.ptr(dh_pl), None, _lib.ptr(dgrid), 0, 0)
                # (the scatter reads a g plane next to dh whatever gn is; with gn == NULL it is multiplied by zero: dh stands in)
        finally:
            meta.lotd.n_active_levels = prev
        if _lib.TIMER is not None:
            _lib.TIMER.note_units("nsim_ngp_bwd", S)
            if dgrid is not None:
                _lib.TIMER.note_units("nsim_lotd_scatter", S)
        if gr is None:      # no consumer of the colour: the radiance network is not part of the graph (None, not zeros)
            drad_w = drad_b = dha = None
        return (None, dgrid, dden_w, dden_b, drad_w, drad_b, dha, d_x, d_o, d_d) + (None,) * 4


class LoTDNeRFModel(ModelMixin, nn.Module):
    is_ray_query_supported = True

    @property
    def ray_query_cfg(self):
        return self._ray_query_cfg

    @ray_query_cfg.setter
    def ray_query_cfg(self, cfg):
        object.__setattr__(self, "_ray_query_cfg", _QueryCfg(cfg or {}))

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

        def lin(o, i):
            b = 1.0 / (i ** 0.5)
            return (torch.rand(o, i, generator=g) * 2 - 1) * b, (torch.rand(o, generator=g) * 2 - 1) * b
        dw1, db1 = lin(64, F + 3)
        dw2, db2 = lin(32, 64)
        rw1, rb1 = lin(64, 47 + NA)
        rw2, rb2 = lin(64, 64)
        rw3, rb3 = lin(3, 64)
        self.den_w = nn.Parameter(torch.cat([dw1.reshape(-1), dw2.reshape(-1)]))
        self.den_b = nn.Parameter(torch.cat([db1, db2]))
        self.rad_w = nn.Parameter(torch.cat([rw1.reshape(-1), rw2.reshape(-1), rw3.reshape(-1)]))
        self.rad_b = nn.Parameter(torch.cat([rb1, rb2, rb3]))
        acc = c["accel_cfg"]
        ufn = acc.get("update_from_net_cfg") or {}
        self.accel = DensityOccGridAccel(
            aabb, resolution=acc.get("resolution", (64, 64, 64)), occ_thre=float(acc.get("occ_thre", 0.01)),
            ema_decay=float(acc.get("ema_decay", 0.95)), num_steps=int(ufn.get("num_steps", 4)),
            num_pts=int(ufn.get("num_pts", 2 ** 20)), n_steps_between_update=int(acc.get("n_steps_between_update", 16)),
            n_steps_warmup=int(acc.get("n_steps_warmup", 256)), update_from_samples_cfg=acc.get("update_from_samples_cfg", None),
            init_cfg=acc.get("init_cfg"), occ_thre_consider_mean=bool(acc.get("occ_thre_consider_mean", False)),
            constant_value=float((acc.get("init_cfg") or {}).get("constant_value", 1.0)))
        self.accel.init()
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
        from ..spatial import AABBSpace
        a = self.accel.aabb
        key = (a.data_ptr(), a._version, str(a.device))
        sp = getattr(self, "_space", None)
        if sp is None or sp[0] != key:
            sp = (key, AABBSpace(aabb=a.detach().clone(), device=a.device))
            object.__setattr__(self, "_space", sp)
        return sp[1]

    # ------------------------------------------------------------------ kernels' inputs
    def _shadow(self):
        """(fp16 table shadow, MFMA-fragment weight pack), refreshed lazily when a parameter changed in place."""
        grid16 = self.encoding.shadow()
        vers = (self.den_w._version, self.den_b._version, self.rad_w._version, self.rad_b._version, self.meta.precision,
                str(self.den_w.device), self.den_w.data_ptr())
        if self._wpack is None or self._wpack_versions != vers:
            nbytes = int(_lib.get_lib().nsim_ngp_wpack_bytes(self.meta))
            if self._wpack is None or self._wpack.numel() != nbytes or self._wpack.device != self.den_w.device:
                self._wpack = torch.zeros([nbytes], dtype=torch.uint8, device=self.den_w.device)
            _lib.call("nsim_ngp_pack_weights", self.meta, _lib.ptr(self.den_w.detach()), _lib.ptr(self.den_b.detach()),
                      _lib.ptr(self.rad_w.detach()), _lib.ptr(self.rad_b.detach()), _lib.ptr(self._wpack))
            self._wpack_versions = vers
        return grid16, self._wpack

    def _gather(self, grid16, x, rays_o, rays_d, t, ridx, S, dev):
        """Level-major f32 feature planes [16][P][2] of S points (``nsim_lotd_gather_lm`` on the f32 meta: features only,
        no dh/dx planes -- the rays get no gradient); the backward reads the same planes."""
        h_pl = torch.empty([16, _lib.plane_pitch(S), 2], dtype=torch.float32, device=dev)
        _lib.call("nsim_lotd_gather_lm", self._fm32, _lib.ptr(grid16), _lib.ptr(x), _lib.ptr(rays_o), _lib.ptr(rays_d),
                  _lib.ptr(t), _lib.ptr(ridx), None, S, None, 0, _lib.ptr(h_pl))
        return h_pl

    def _step(self, cfg: dict = None) -> float:
        qp = (cfg or {}).get("query_param", None) or self.ray_query_cfg.get("query_param", {})
        return float((qp.get("march_cfg") or {}).get("step_size", 0.1))

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

    def ray_query(self, *, ray_input: dict = None, ray_tested: dict, config=None, return_buffer: bool = True,
                  return_details: bool = False, render_per_obj_individual: bool = False, with_rgb: bool = None,
                  with_normal: bool = None, **unused) -> Dict:
        """``query_mode: march_occ``: the samples are the marcher's lattice t_k = near + (k + jitter) step inside occupied
        voxels (jitter per ray when ``perturb``, else 0); every sample's interval is ``step``."""
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
        has_grad = rays_has_grad(self.ray_query_cfg, cfg)
        for k in ("rays_o", "rays_d"):
            if ray_tested[k].requires_grad and not has_grad:
                raise NotImplementedError(f"ray_tested[{k!r}].requires_grad: gradients to rays (pose refinement) are not built "
                                          f"for this model unless ray_query_cfg.query_param.rays_has_grad is set")
        # marching, the occupancy grid and the sample depths see detached rays; the decoders' samples o + t d carry the graph
        o = ray_tested["rays_o"].detach().float().contiguous()
        d = ray_tested["rays_d"].detach().float().contiguous()
        o_g = ray_tested["rays_o"].float().contiguous() if ray_tested["rays_o"].requires_grad else o
        d_g = ray_tested["rays_d"].float().contiguous() if ray_tested["rays_d"].requires_grad else d
        near, far = ray_tested["near"].detach().float().contiguous(), ray_tested["far"].detach().float().contiguous()
        dev = o.device
        jitter = cfg.get("_jitter", None)
        if jitter is None:
            jitter = torch.rand([R], device=dev) if cfg.get("perturb", False) else torch.zeros([R], device=dev)
        jitter = jitter.float().contiguous()
        bits, occm = self.accel.occ_bits, self.accel.meta
        with torch.no_grad():
            counts = torch.empty([R], dtype=torch.long, device=dev)
            _lib.call("nsim_march_count", _lib.ptr(o), _lib.ptr(d), _lib.ptr(near), _lib.ptr(far), _lib.ptr(jitter), R,
                      _lib.ptr(bits), None, occm, step, max_steps, _lib.ptr(counts))
            pi, total = po.get_pack_infos_from_n(counts, return_total=True)
            S = int(total.item())                    # host sync: size of the marched set
            if S == 0:
                self.accel.collect_armed = False
                return empty(dict(march_counts=counts))
            t = torch.empty([S], dtype=torch.float32, device=dev)
            _lib.call("nsim_march_emit", _lib.ptr(o), _lib.ptr(d), _lib.ptr(near), _lib.ptr(far), _lib.ptr(jitter), R,
                      _lib.ptr(bits), None, occm, step, max_steps, _lib.ptr(pi), _lib.ptr(t))
            ridx = torch.repeat_interleave(torch.arange(R, device=dev), counts, output_size=S)
            sel = counts.nonzero()[:, 0]
        h_appear = ray_tested.get("rays_h_appear", None) if (with_rgb and self.n_appear) else None
        if with_rgb and self.n_appear and h_appear is None:
            raise ValueError("ray_tested['rays_h_appear'] is missing: radiance_decoder_cfg.n_appear_embedding is "
                             f"{self.n_appear}, the radiance decoder reads a per-ray appearance code")
        outs = _NgpFn.apply(self, self.encoding.flattened_params, self.den_w, self.den_b, self.rad_w, self.rad_b, h_appear,
                            None, o_g, d_g, t, ridx, step, bool(with_rgb))
        sigma, alpha = outs[0], outs[1]
        if self.accel.collect_armed:
            self.accel.collect(sigma=sigma, rays=(o, d, t, ridx))
            self.accel.collect_armed = False
        vb = dict(type="packed", rays_inds_hit=ray_tested["rays_inds"][sel], pack_infos_hit=pi[sel], t=t, sigma=sigma,
                  opacity_alpha=alpha)
        if with_rgb:
            vb["rgb"] = outs[2]
        ret = dict(volume_buffer=vb)
        if render_per_obj_individual or cfg.get("_render", False):
            from .neus import volume_integration
            ret["rendered"] = volume_integration(alpha, t, outs[2] if with_rgb else None, None, pi,
                                                 cfg.get("depth_use_normalized_vw", True),
                                                 rays_inds=ray_tested["rays_inds"] if n_all is not None else None, num_rays=n_all)
            ret["rendered"].pop("vw", None)
            ret["rendered"].pop("trans", None)
        if return_details:
            ret["details"] = dict(march_counts=counts, ridx=ridx, pack_infos=pi)
        return ret
