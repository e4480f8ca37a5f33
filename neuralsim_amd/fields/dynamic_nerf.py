"""Dynamic-only EmerNeRF street model -- host side of csrc/nerf_field.hip's ``k_dyn`` kernels.

Mirrors ``nr3d_lib.models.fields_dynamic.nerf.EmerNeRFOnlyDynamicModel`` as the reference wraps and drives it
(``EmerNerfStreetOnlyDynamic``, app/models/single/dynamic_nerf.py:93-160; config
code_multi/configs/exps/fg_neus=permuto_emernerf/with_gtbox.240212.yaml:277-370): a density NeRF over (x, y, z, time) on a 4-D
permutohedral lattice with a time-sliced occupancy grid.  The implementation lives in the absent nr3d_lib: the semantics are
this package's reading of the yaml, recorded in DESIGN.md sec. 7; tests/dynamic_nerf_ref.py is the executable spec.

All arithmetic runs in HIP kernels: the lattice gather / scatter of csrc/permuto.hip (``nsim_permuto_gather_pts`` /
``_scatter_pts``), the occupancy marcher of csrc/sampling.hip with a per-ray word offset, and the fused decoders, the time
input and the time-sliced occupancy folds of csrc/nerf_field.hip.  This file allocates tensors, sequences launches and defines
the autograd boundary.

``use_flow_field: true`` (code_multi/configs/exps/fg_emernerf/no_gtbox_with_flow.240208.yaml:353-371): a second 4-D lattice and a
flow decoder (``nsim_flow_fwd`` / ``_bwd``) predict the forward / backward scene flow; the density decoder aggregates its hidden
features over the sample and its two flow-warped neighbours (``nsim_dyn_fwd_agg`` / ``_bwd_agg``), and the gradient reaches the
flow through the warped lattice points (``nsim_permuto_dx_pts``, ``nsim_dyn_warp_bwd``).  tests/dynamic_flow_ref.py is that
variant's executable spec.
"""
from typing import Dict, Optional

import torch

from .. import _lib
from ..grid_encodings.permuto import PermutoConfig
from ..spatial import aabb_ray_test
from .density_base import MarchedDensityModel, f32c, reduce_ray_grads, zero_grads_like
from .nerf import DensityOccGridAccel
from .neus import _QueryCfg
from .permuto_neus import _PermutoFieldEncoding


class DynamicDensityOccGridAccel(DensityOccGridAccel):
    """``accel_cfg{type: occ_grid_dynamic, vox_size | resolution, occ_thre, occ_thre_consider_mean, ema_decay, init_cfg{mode:
    constant, constant_value}, update_from_net_cfg, update_from_samples_cfg: {}, n_steps_between_update, n_steps_warmup,
    ts_keyframes}`` (with_gtbox.240212.yaml:339-354): K = len(ts_keyframes) density value grids of one resolution over the
    model's AABB, one per accelerator keyframe.  ``occ_val`` is [K * n_voxels], ``occ_bits`` [K * ceil(n_voxels / 32)]; a ray
    marches the slice whose keyframe is nearest to its time (``ray_word_off``).  Slice by slice it behaves as K independent
    ``DensityOccGridAccel``s, each fed that slice's points."""

    def __init__(self, aabb, ts_keyframes, **kw):
        dev = kw.pop("device", None)
        super().__init__(aabb, **kw)
        ts = torch.as_tensor(ts_keyframes, dtype=torch.float32).detach().reshape(-1).clone()
        assert ts.numel() >= 1 and bool((ts[1:] > ts[:-1]).all()), "accelerator keyframes must ascend"
        self.K = int(ts.numel())
        self.nvox = self.resolution[0] * self.resolution[1] * self.resolution[2]
        self.words_per_slice = (self.nvox + 31) // 32
        self.register_buffer("ts_keyframes", ts)
        self.register_buffer("occ_val", torch.zeros(self.K * self.nvox, dtype=torch.float32))
        self.register_buffer("occ_bits", torch.full([self.K * self.words_per_slice], -1, dtype=torch.int32))
        self.register_buffer("occ_thre_dev", torch.full([self.K], self.occ_thre, dtype=torch.float32))
        self.register_buffer("_mean_ws", torch.zeros([65 * self.K], dtype=torch.float32), persistent=False)
        if dev is not None:
            self.to(dev)

    # ------------------------------------------------------------------ slices
    def _time_call(self, ts, slice_out, off_out):
        ts = ts.detach().float().reshape(-1).contiguous()
        _lib.call("nsim_dyn_time", _lib.ptr(self.ts_keyframes), None, self.K, _lib.ptr(ts), ts.shape[0],
                  self.words_per_slice, None, _lib.ptr(slice_out), _lib.ptr(off_out))

    def slice_of(self, ts: torch.Tensor) -> torch.Tensor:
        """int64 [n]: the accelerator keyframe nearest to each time (a tie to the lower index, the ends clamp)."""
        out = torch.empty([ts.numel()], dtype=torch.long, device=self.occ_val.device)
        self._time_call(ts, out, None)
        return out

    def ray_word_off(self, ts: torch.Tensor) -> torch.Tensor:
        """int64 [n]: ``slice_of(ts) * words_per_slice``, the marcher's per-ray word offset into ``occ_bits``."""
        out = torch.empty([ts.numel()], dtype=torch.long, device=self.occ_val.device)
        self._time_call(ts, None, out)
        return out

    def _occupied(self) -> torch.Tensor:
        """bool [K, n_voxels] in storage order: the bits the marcher reads."""
        sh = torch.arange(32, dtype=torch.int32, device=self.occ_bits.device)
        b = ((self.occ_bits.view(self.K, -1, 1) >> sh) & 1).bool()
        return b.reshape(self.K, -1)[:, :self.nvox]

    @property
    def occ_grid(self) -> torch.Tensor:
        r = self.resolution
        return self._occupied().view(self.K, r[2], r[1], r[0]).permute(0, 3, 2, 1)

    def frac_occupied(self, per_slice: bool = False):
        f = self._occupied().float().mean(dim=1)
        return f if per_slice else float(f.mean())

    def set_all_occupied(self):
        self.occ_val.fill_(max(self.constant_value, 2.0 * self.occ_thre, 1e-30))
        self.occ_bits.fill_(-1)
        self._clear_padding()

    def _clear_padding(self):
        """``fill_(-1)`` sets the padding bits of a slice's last word as well: they are never set."""
        tail = self.nvox & 31
        if tail:
            self.occ_bits.view(self.K, -1)[:, -1] = (1 << tail) - 1

    def pack_bits(self):
        _lib.call("nsim_occ_pack_bits_mean_sliced", _lib.ptr(self.occ_val), self.nvox, self.nvox, self.K, self.occ_thre,
                  int(self.occ_thre_consider_mean), _lib.ptr(self._mean_ws), _lib.ptr(self.occ_bits))
        self.occ_thre_dev = self._mean_ws.view(self.K, 65)[:, 64].clone()

    @torch.no_grad()
    def update_from_samples(self, pts, sigma, slices, pack=True):
        """Every slice decays once (val * ema_decay); point i is max-folded into slice ``slices[i]``."""
        pts = pts.detach().float().contiguous()
        sigma = sigma.detach().float().contiguous()
        slices = slices.detach().long().contiguous()
        _lib.call("nsim_occ_update_density_sliced", _lib.ptr(self.occ_val), self.nvox, self.nvox, self.K, self.ema_decay,
                  _lib.ptr(pts), _lib.ptr(sigma), _lib.ptr(slices), pts.shape[0], self.meta)
        if pack:
            self.pack_bits()

    def update_from_net(self, query_density, num_steps=None, num_pts=None, generator=None):
        """``update_from_net_cfg{num_steps, num_pts}``: per step ``draw_points(num_pts)`` and a random slice per point from
        the same generator; the density is queried at (pts, ts_keyframes[slice])."""
        if self.update_from_samples_cfg is not None and self.sync_values is not None:
            self.sync_values(self.occ_val)
        dev = self.occ_val.device
        for _ in range(num_steps or self.num_steps):
            n = num_pts or self.num_pts
            pts = self.draw_points(n, generator)
            k = torch.randint(self.K, [n], device=dev, generator=generator)
            self.update_from_samples(pts, query_density(pts, self.ts_keyframes[k]), k, pack=False)
        self.pack_bits()

    @torch.no_grad()
    def collect(self, sigma, slices, pts=None, rays=None):
        """Max-fold the densities of a training step's own samples into their slices (no decay, bits untouched): ``pts``
        [n,3] with ``slices`` [n], or ``rays`` = (rays_o, rays_d, t, ridx) with ``slices`` per ray."""
        o, d, t, ridx = rays if rays is not None else (None, None, None, None)
        _lib.call("nsim_occ_collect_density_sliced", _lib.ptr(self.occ_val), self.nvox, self.K, _lib.ptr(pts), _lib.ptr(o),
                  _lib.ptr(d), _lib.ptr(t), _lib.ptr(ridx), _lib.ptr(slices.detach().long().contiguous()),
                  _lib.ptr(sigma.detach().float().contiguous()), sigma.shape[0], self.meta)

    def init(self, query_density=None, logger=None, **kw):
        """``init_cfg{mode: constant, constant_value}``: every slice holds the constant and is fully occupied."""
        self.occ_val.fill_(self.constant_value)
        self.occ_bits.fill_(-1)
        self._clear_padding()
        self.occ_thre_dev = torch.full_like(self.occ_thre_dev, min(self.occ_thre, self.constant_value)
                                            if self.occ_thre_consider_mean else self.occ_thre)


class _DynFn(torch.autograd.Function):
    """(table, den_w, den_b, rad_w, rad_b, h_appear) -> (sigma [S], alpha [S] [, rgb [S,3]]) at the lattice points x4 [S,4]:
    level-major lattice gather, then the fused decoders on the planes.  ``p_x`` [S,3] | ``p_o``, ``p_d`` [R,3] with ``p_t`` [S]: the
    points or rays x4 was made of, given only when they carry gradients (pose refinement, ``rays_has_grad``): the backward then
    returns theirs -- ``nsim_dyn_bwd_pose`` (dv) -> ``nsim_permuto_dx_pts`` -> ``nsim_dyn_pose_dx`` -> ``nsim_ray_grad_reduce``."""

    @staticmethod
    def forward(ctx, model, grid, den_w, den_b, rad_w, rad_b, h_appear, x4, rays_d, ridx, step, with_rgb, p_x=None, p_o=None,
                p_d=None, p_t=None):
        dev = grid.device
        S = x4.shape[0]
        grid16, wpack = model._shadow()
        need_bwd = any(ctx.needs_input_grad)
        h_pl = torch.empty([16, S, 2], dtype=torch.float32, device=dev)
        _lib.call("nsim_permuto_gather_pts", model.encoding.cfg.pmeta, _lib.ptr(grid16), _lib.ptr(x4), S, _lib.ptr(h_pl))
        sigma = torch.empty([S], dtype=torch.float32, device=dev)
        alpha = torch.empty([S], dtype=torch.float32, device=dev)
        rgb = torch.empty([S, 3], dtype=torch.float32, device=dev) if with_rgb else None
        ha = h_appear.detach().float().contiguous() if (h_appear is not None and with_rgb and model.n_appear) else None
        _lib.call("nsim_dyn_fwd", model.meta, _lib.ptr(wpack), _lib.ptr(h_pl), S, _lib.ptr(rays_d if with_rgb else None),
                  _lib.ptr(ridx if with_rgb else None), _lib.ptr(ha), S, float(step), _lib.ptr(sigma), _lib.ptr(alpha),
                  _lib.ptr(rgb))
        if _lib.TIMER is not None:
            _lib.TIMER.note_units("nsim_dyn_fwd", S)
        ctx.model, ctx.S, ctx.step, ctx.with_rgb = model, S, float(step), with_rgb
        ctx.n_active = int(model.meta.lotd.n_active_levels)
        ctx.ha_shape = h_appear.shape if ha is not None else None
        ctx.ray_shape = p_o.shape if p_o is not None else (p_d.shape if p_d is not None else None)
        ctx.set_materialize_grads(False)
        pose_in = p_x is not None or p_o is not None or p_d is not None       # (the table the forward read: the backward's dx_pts)
        ctx.save_for_backward(x4, rays_d, ridx, ha, h_pl if need_bwd else None, sigma, rgb, p_t, grid16 if pose_in else None)
        return (sigma, alpha, rgb) if with_rgb else (sigma, alpha)

    @staticmethod
    def backward(ctx, g_sigma, g_alpha, g_rgb=None):
        model = ctx.model
        x4, rays_d, ridx, ha, h_pl, sigma, rgb, p_t, grid16 = ctx.saved_tensors
        n_out = len(ctx.needs_input_grad)       # 12, or 16 with the pose inputs
        need = tuple(ctx.needs_input_grad) + (False,) * (16 - n_out)
        if g_sigma is None and g_alpha is None and g_rgb is None:
            return (None,) * n_out
        dev, S = sigma.device, ctx.S
        wpack = model._shadow()[1]
        dden_w, dden_b, drad_w, drad_b = zero_grads_like(model.den_w, model.den_b, model.rad_w, model.rad_b)
        gs, ga, gr = f32c(g_sigma), f32c(g_alpha), f32c(g_rgb if ctx.with_rgb else None)
        dha = _lib.zeros(list(ctx.ha_shape), device=dev) if (ha is not None and need[6] and gr is not None) else None
        dgrid = _lib.zeros([model.encoding.cfg.n_params], device=dev) if need[1] else None
        need_x, need_o, need_d = need[12], need[13], need[14]
        pose = need_x or need_o or need_d
        dh_pl = torch.empty([16, S, 2], dtype=torch.float32, device=dev) if (dgrid is not None or pose) else None
        dv = torch.empty([S, 3], dtype=torch.float32, device=dev) if (need_d and gr is not None) else None
        d_x = d_o = d_d = None
        with model._level_mask(ctx.n_active):
            args = (model.meta, _lib.ptr(wpack), _lib.ptr(h_pl), S, _lib.ptr(rays_d if gr is not None else None),
                    _lib.ptr(ridx if gr is not None else None), _lib.ptr(ha), S, ctx.step, _lib.ptr(sigma.detach()),
                    _lib.ptr(rgb.detach()) if rgb is not None else None, _lib.ptr(gs), _lib.ptr(ga), _lib.ptr(gr),
                    _lib.ptr(dh_pl), _lib.ptr(dden_w), _lib.ptr(dden_b), _lib.ptr(drad_w), _lib.ptr(drad_b), _lib.ptr(dha))
            if dv is not None:
                _lib.call("nsim_dyn_bwd_pose", *args, _lib.ptr(dv))
            else:
                _lib.call("nsim_dyn_bwd", *args)
            if pose:
                dx4 = torch.empty([S, 4], dtype=torch.float32, device=dev)
                _lib.call("nsim_permuto_dx_pts", model.encoding.cfg.pmeta, _lib.ptr(grid16), _lib.ptr(x4), None, S,
                          _lib.ptr(dh_pl), 0, _lib.ptr(dx4))
                dx = torch.empty([S, 3], dtype=torch.float32, device=dev)
                _lib.call("nsim_dyn_pose_dx", _lib.ptr(dx4), None, None, None, S, _lib.ptr(dx))
                d_x, d_o, d_d = reduce_ray_grads(dx, dv, p_t, ridx, ctx.ray_shape, need_x, need_o, need_d)
            if dgrid is not None:
                _lib.call("nsim_permuto_scatter_pts", model.encoding.cfg.pmeta, _lib.ptr(x4), _lib.ptr(_all_valid(S, dev)), S,
                          _lib.ptr(dh_pl), _lib.ptr(dgrid))
        if _lib.TIMER is not None:
            _lib.TIMER.note_units("nsim_dyn_bwd", S)
            if dgrid is not None:
                _lib.TIMER.note_units("nsim_permuto_scatter_pts", S)
        if gr is None:      # no consumer of the colour: the radiance network is not part of the graph (None, not zeros)
            drad_w = drad_b = dha = None
        return ((None, dgrid, dden_w, dden_b, drad_w, drad_b, dha) + (None,) * 5 + (d_x, d_o, d_d, None))[:n_out]


FLOW_KEYS = ("flow_fwd", "flow_fwd_pred_bwd", "flow_bwd", "flow_bwd_pred_fwd")


def _all_valid(n, dev):
    return torch.ones([n], dtype=torch.uint8, device=dev)


class _DynFlowFn(torch.autograd.Function):
    """The with-flow query (``use_flow_field``): (table, den_w, den_b, rad_w, rad_b, h_appear, flow table, flow_w, flow_b) ->
    (sigma [S], alpha [S], rgb [S,3] | None, flow6 [S,6], pred6 [2S,6]) at the lattice points x4 [S,4].  Flow at x -> warp -> flow at
    the 2S warped points -> dynamic gather at the 3S points -> aggregating decoder.  flow6 = (flow_fwd | flow_bwd) at x; pred6 rows
    0..S are the flow at (x+, w+), rows S..2S at (x-, w-).  The backward carries d loss / d x+- from both lattices into the flow at
    x (``nsim_permuto_dx_pts`` -> ``nsim_dyn_warp_bwd``); times get no gradient.  ``p_x`` | ``p_o``, ``p_d``, ``p_t`` as in
    ``_DynFn``: with them the backward also returns the gradient to the points or rays -- per sample the position parts of the
    dynamic lattice's gradient at x, of both lattices' at x+ and x- (d x+- / d x = I) and of the flow lattice's at x under the
    total dflow6 (``nsim_dyn_pose_dx``), dv from ``nsim_dyn_bwd_agg_pose``; then ``nsim_ray_grad_reduce``."""

    @staticmethod
    def forward(ctx, model, grid, den_w, den_b, rad_w, rad_b, h_appear, fgrid, flow_w, flow_b, x4, rays_d, ridx, step, with_rgb,
                p_x=None, p_o=None, p_d=None, p_t=None):
        dev, S = grid.device, x4.shape[0]
        grid16, wpack = model._shadow()
        fgrid16, fwpack = model._flow_shadow()
        fm, dm = model.flow_encoding.cfg.pmeta, model.encoding.cfg.pmeta
        Lf, prec = int(fm.num_levels), int(model.meta.precision)
        lo, hi = model.cfgd["time_range"]
        hf = torch.empty([16, S, 2], dtype=torch.float32, device=dev)
        _lib.call("nsim_permuto_gather_pts", fm, _lib.ptr(fgrid16), _lib.ptr(x4), S, _lib.ptr(hf))
        flow6 = torch.empty([S, 6], dtype=torch.float32, device=dev)
        _lib.call("nsim_flow_fwd", Lf, prec, _lib.ptr(fwpack), _lib.ptr(hf), 0, S, _lib.ptr(flow6))
        x4all = torch.empty([3 * S, 4], dtype=torch.float32, device=dev)
        x4all[:S] = x4
        x4w = x4all[S:]
        _lib.call("nsim_dyn_warp_fwd", _lib.ptr(x4), _lib.ptr(flow6), S, float(model.time_delta), float(lo), float(hi), _lib.ptr(x4w))
        hfw = torch.empty([16, 2 * S, 2], dtype=torch.float32, device=dev)
        _lib.call("nsim_permuto_gather_pts", fm, _lib.ptr(fgrid16), _lib.ptr(x4w), 2 * S, _lib.ptr(hfw))
        pred6 = torch.empty([2 * S, 6], dtype=torch.float32, device=dev)
        _lib.call("nsim_flow_fwd", Lf, prec, _lib.ptr(fwpack), _lib.ptr(hfw), 0, 2 * S, _lib.ptr(pred6))
        h_pl = torch.empty([16, 3 * S, 2], dtype=torch.float32, device=dev)
        _lib.call("nsim_permuto_gather_pts", dm, _lib.ptr(grid16), _lib.ptr(x4all), 3 * S, _lib.ptr(h_pl))
        sigma = torch.empty([S], dtype=torch.float32, device=dev)
        alpha = torch.empty([S], dtype=torch.float32, device=dev)
        rgb = torch.empty([S, 3], dtype=torch.float32, device=dev) if with_rgb else None
        ha = h_appear.detach().float().contiguous() if (h_appear is not None and with_rgb and model.n_appear) else None
        _lib.call("nsim_dyn_fwd_agg", model.meta, _lib.ptr(wpack), _lib.ptr(h_pl), _lib.ptr(rays_d if with_rgb else None),
                  _lib.ptr(ridx if with_rgb else None), _lib.ptr(ha), S, float(step), _lib.ptr(sigma), _lib.ptr(alpha), _lib.ptr(rgb))
        if _lib.TIMER is not None:
            _lib.TIMER.note_units("nsim_dyn_fwd_agg", S)
        ctx.model, ctx.S, ctx.step, ctx.with_rgb = model, S, float(step), with_rgb
        ctx.n_active = int(model.meta.lotd.n_active_levels)
        ctx.ha_shape = h_appear.shape if ha is not None else None
        ctx.set_materialize_grads(False)
        need_bwd = any(ctx.needs_input_grad)
        ctx.ray_shape = p_o.shape if p_o is not None else (p_d.shape if p_d is not None else None)
        ctx.save_for_backward(x4all, rays_d, ridx, ha, sigma, rgb, p_t, *((h_pl, hf, hfw, grid16, fgrid16) if need_bwd else ()))
        if with_rgb:
            return sigma, alpha, rgb, flow6, pred6
        return sigma, alpha, flow6, pred6

    @staticmethod
    def backward(ctx, g_sigma, g_alpha, *rest):
        model, S = ctx.model, ctx.S
        g_rgb, g_flow6, g_pred6 = (rest if ctx.with_rgb else (None,) + tuple(rest))
        n_out = len(ctx.needs_input_grad)       # 15, or 19 with the pose inputs
        if all(g is None for g in (g_sigma, g_alpha, g_rgb, g_flow6, g_pred6)):
            return (None,) * n_out
        x4all, rays_d, ridx, ha, sigma, rgb, p_t, h_pl, hf, hfw, grid16, fgrid16 = ctx.saved_tensors
        dev = sigma.device
        need_x, need_o, need_d = (tuple(ctx.needs_input_grad) + (False,) * 4)[15:18]
        pose = need_x or need_o or need_d
        dv = dx_a = dx_dyn = dx_flow = None
        x4, x4w = x4all[:S], x4all[S:]
        wpack, fwpack = model._shadow()[1], model._flow_shadow()[1]
        fm, dm = model.flow_encoding.cfg.pmeta, model.encoding.cfg.pmeta
        Lf, prec = int(fm.num_levels), int(model.meta.precision)
        dden_w, dden_b, drad_w, drad_b = zero_grads_like(model.den_w, model.den_b, model.rad_w, model.rad_b)
        dflow_w, dflow_b = zero_grads_like(model.flow_w, model.flow_b)
        dgrid = _lib.zeros([model.encoding.cfg.n_params], device=dev)
        dfgrid = _lib.zeros([model.flow_encoding.cfg.n_params], device=dev)
        dflow6 = g_flow6.float().contiguous().clone() if g_flow6 is not None else _lib.zeros([S, 6], device=dev)
        gr = f32c(g_rgb if ctx.with_rgb else None)
        dha = _lib.zeros(list(ctx.ha_shape), device=dev) if (ha is not None and ctx.needs_input_grad[6] and gr is not None) else None
        dense_grad = not (g_sigma is None and g_alpha is None and gr is None)
        if dense_grad:
            gs, ga = f32c(g_sigma), f32c(g_alpha)
            dh_pl = torch.empty([16, 3 * S, 2], dtype=torch.float32, device=dev)
            dx_dyn = torch.empty([2 * S, 4], dtype=torch.float32, device=dev)
            with model._level_mask(ctx.n_active):
                args = (model.meta, _lib.ptr(wpack), _lib.ptr(h_pl), _lib.ptr(rays_d if gr is not None else None),
                        _lib.ptr(ridx if gr is not None else None), _lib.ptr(ha), S, ctx.step, _lib.ptr(sigma.detach()),
                        _lib.ptr(rgb.detach()) if rgb is not None else None, _lib.ptr(gs), _lib.ptr(ga), _lib.ptr(gr),
                        _lib.ptr(dh_pl), _lib.ptr(dden_w), _lib.ptr(dden_b), _lib.ptr(drad_w), _lib.ptr(drad_b), _lib.ptr(dha))
                if need_d and gr is not None:
                    dv = torch.empty([S, 3], dtype=torch.float32, device=dev)
                    _lib.call("nsim_dyn_bwd_agg_pose", *args, _lib.ptr(dv))
                else:
                    _lib.call("nsim_dyn_bwd_agg", *args)
                if pose:        # the un-warped rows of the same planes
                    dx_a = torch.empty([S, 4], dtype=torch.float32, device=dev)
                    _lib.call("nsim_permuto_dx_pts", dm, _lib.ptr(grid16), _lib.ptr(x4), None, S, _lib.ptr(dh_pl), 3 * S, _lib.ptr(dx_a))
                _lib.call("nsim_permuto_scatter_pts", dm, _lib.ptr(x4all), _lib.ptr(_all_valid(3 * S, dev)), 3 * S, _lib.ptr(dh_pl),
                          _lib.ptr(dgrid))
                # the plane sets of the warped points start S rows into every level of the [16][3S][2] buffer
                _lib.call("nsim_permuto_dx_pts", dm, _lib.ptr(grid16), _lib.ptr(x4w), None, 2 * S, _lib.ptr(dh_pl.view(-1)[2 * S:]),
                          3 * S, _lib.ptr(dx_dyn))
            _lib.call("nsim_dyn_warp_bwd", _lib.ptr(dx_dyn), S, _lib.ptr(dflow6))
            if _lib.TIMER is not None:
                _lib.TIMER.note_units("nsim_dyn_bwd_agg", S)
        if g_pred6 is not None:
            dh_fw = torch.empty([16, 2 * S, 2], dtype=torch.float32, device=dev)
            _lib.call("nsim_flow_bwd", Lf, prec, _lib.ptr(fwpack), _lib.ptr(hfw), 0, 2 * S, _lib.ptr(g_pred6.float().contiguous()),
                      _lib.ptr(dh_fw), _lib.ptr(dflow_w), _lib.ptr(dflow_b))
            _lib.call("nsim_permuto_scatter_pts", fm, _lib.ptr(x4w), _lib.ptr(_all_valid(2 * S, dev)), 2 * S, _lib.ptr(dh_fw),
                      _lib.ptr(dfgrid))
            dx_flow = torch.empty([2 * S, 4], dtype=torch.float32, device=dev)
            _lib.call("nsim_permuto_dx_pts", fm, _lib.ptr(fgrid16), _lib.ptr(x4w), None, 2 * S, _lib.ptr(dh_fw), 0, _lib.ptr(dx_flow))
            _lib.call("nsim_dyn_warp_bwd", _lib.ptr(dx_flow), S, _lib.ptr(dflow6))
        dh_f = torch.empty([16, S, 2], dtype=torch.float32, device=dev)
        _lib.call("nsim_flow_bwd", Lf, prec, _lib.ptr(fwpack), _lib.ptr(hf), 0, S, _lib.ptr(dflow6), _lib.ptr(dh_f), _lib.ptr(dflow_w),
                  _lib.ptr(dflow_b))
        _lib.call("nsim_permuto_scatter_pts", fm, _lib.ptr(x4), _lib.ptr(_all_valid(S, dev)), S, _lib.ptr(dh_f), _lib.ptr(dfgrid))
        d_x = d_o = d_d = None
        if pose:            # the total dflow6 pulled back through the flow field at x, and the sum of the position parts
            dx_f = torch.empty([S, 4], dtype=torch.float32, device=dev)
            _lib.call("nsim_permuto_dx_pts", fm, _lib.ptr(fgrid16), _lib.ptr(x4), None, S, _lib.ptr(dh_f), 0, _lib.ptr(dx_f))
            dx = torch.empty([S, 3], dtype=torch.float32, device=dev)
            _lib.call("nsim_dyn_pose_dx", _lib.ptr(dx_a), _lib.ptr(dx_f), _lib.ptr(dx_dyn), _lib.ptr(dx_flow), S, _lib.ptr(dx))
            d_x, d_o, d_d = reduce_ray_grads(dx, dv, p_t, ridx, ctx.ray_shape, need_x, need_o, need_d)
        if gr is None:      # no consumer of the colour: the radiance network is not part of the graph (None, not zeros)
            drad_w = drad_b = dha = None
        return ((None, dgrid, dden_w, dden_b, drad_w, drad_b, dha, dfgrid, dflow_w, dflow_b) + (None,) * 5 + (d_x, d_o, d_d, None))[:n_out]


class EmerNeRFOnlyDynamicModel(MarchedDensityModel):
    use_ts = True
    use_view_dirs = True
    _appear_cfg = "radiance_cfg"

    def __init__(self, aabb: torch.Tensor = None, ts_keyframes: torch.Tensor = None, seed: int = 42, device=None,
                 accel_n_jump_frames: int = None, **model_params):
        """``model_params``: the reference's yaml block verbatim (with_gtbox.240212.yaml:279-360; fields/ref_config.py
        ``validate_emernerf_params`` names every option the kernels do not cover).  The lattice normalisation, the keyframe
        codes and the time-sliced occupancy grid need the AABB and the keyframe times: built by ``populate(aabb=,
        ts_keyframes=)`` (app/models/single/dynamic_nerf.py:153)."""
        super().__init__()
        from . import ref_config
        self._params, self._seed = dict(model_params), int(seed)
        self._pending_device = device
        self.cfgd = ref_config.validate_emernerf_params(self._params)
        self.accel_cfg = _QueryCfg(self.cfgd["accel_cfg"])     # (the asset's populate adds ``ts_keyframes`` here, :150)
        self.ray_query_cfg = self.cfgd["ray_query_cfg"]
        self.n_appear = self.cfgd["n_appear"]
        self._n_jump = accel_n_jump_frames
        self._built = False
        if aabb is not None and ts_keyframes is not None:
            self.populate(aabb=aabb, ts_keyframes=ts_keyframes, device=device)

    def _build(self, aabb: torch.Tensor, ts: torch.Tensor, ts_accel: torch.Tensor):
        from . import ref_config
        c = self.cfgd
        pcfg = PermutoConfig(in_dim=4, **c["permuto_auto_compute_cfg"])
        self.encoding = _PermutoFieldEncoding(pcfg, c["param_bound"], self._seed)
        self.encoding.cfg.set_aabb(aabb)        # (x, y, z) normalised by the AABB; the 4th input (time code) as it stands
        F, NA = self.encoding.cfg.out_features, self.n_appear
        g = torch.Generator().manual_seed(self._seed + 1)
        self._make_decoder("den", [(64, F), (65, 64)], g)
        self._make_decoder("rad", [(64, 80 + NA), (64, 64), (3, 64)], g)
        self.use_flow = c.get("flow") is not None
        if self.use_flow:
            # (use_flow_field, no_gtbox_with_flow.240208.yaml:353-371) a second 4-D lattice with its own seed, shifts, table and
            # fp16 shadow, and the [F_f -> 64 -> 64 -> 6] decoder of the forward / backward scene flow
            fl = c["flow"]
            fac = dict(fl["permuto_auto_compute_cfg"])
            fac.setdefault("seed", 1)
            self.flow_encoding = _PermutoFieldEncoding(PermutoConfig(in_dim=4, **fac), fl["param_bound"], self._seed + 2)
            self.flow_encoding.cfg.set_aabb(aabb)
            self._make_decoder("flow", [(64, self.flow_encoding.cfg.out_features), (64, 64), (6, 64)], g)
        T = int(ts.numel())
        self.register_buffer("ts_keyframes", ts.clone())
        lo, hi = c["time_range"]
        self.time_delta = (hi - lo) / (T - 1) if T > 1 else 0.0        # spacing of the keyframe codes: the flow's time step
        self.register_buffer("time_codes", torch.linspace(lo, hi, T, dtype=torch.float32), persistent=False)
        acc = dict(self.accel_cfg)
        acc.pop("ts_keyframes", None)
        self._make_accel(DynamicDensityOccGridAccel, aabb, ts_accel, acc=acc, resolution=ref_config.occ_resolution(acc, aabb))
        m = _lib.NgpMeta()
        m.lotd = self.encoding.cfg.meta         # level count and hardmask of the decoder launches (a stub pyramid)
        m.precision = {"fp16": 0, "f32": 1}[c["precision"]]
        m.n_appear = NA
        self.meta = m
        self._wpack, self._wpack_versions = None, None
        self._fwpack, self._fwpack_versions = None, None
        self._built = True

    # ------------------------------------------------------------------ reference life cycle
    def populate(self, aabb: torch.Tensor = None, ts_keyframes: torch.Tensor = None, device=None,
                 accel_n_jump_frames: int = None, **unused):
        """``populate(aabb=, ts_keyframes=, device=)`` (app/models/single/dynamic_nerf.py:153).  The accelerator's keyframes are
        ``accel_cfg['ts_keyframes']`` when the caller put them there (:150), else ``ts_keyframes[::accel_n_jump_frames]``
        (``populate_cfg.accel_n_jump_frames``, default 2)."""
        device = device if device is not None else self._pending_device
        if aabb is not None or ts_keyframes is not None:
            if aabb is None or ts_keyframes is None:
                raise AssertionError("the dynamic model is sized from the AABB and the keyframe times: populate(aabb=, ts_keyframes=)")
            a = torch.as_tensor(aabb, dtype=torch.float32).reshape(2, 3).detach().cpu()
            ts = torch.as_tensor(ts_keyframes, dtype=torch.float32).reshape(-1).detach().cpu()
            assert ts.numel() >= 1 and bool((ts[1:] > ts[:-1]).all()), "ts_keyframes must ascend"
            tsa = self.accel_cfg.get("ts_keyframes", None)
            if tsa is None:
                nj = accel_n_jump_frames if accel_n_jump_frames is not None else (self._n_jump if self._n_jump is not None else 2)
                tsa = ts[::int(nj)]
            tsa = torch.as_tensor(tsa, dtype=torch.float32).reshape(-1).detach().cpu().contiguous()
            same = self._built and torch.equal(a, self.accel.aabb.cpu()) and torch.equal(ts, self.ts_keyframes.cpu()) and \
                torch.equal(tsa, self.accel.ts_keyframes.cpu())
            if not same:
                self._build(a, ts, tsa)
        elif not self._built:
            raise AssertionError("the dynamic model is sized from the AABB and the keyframe times: populate(aabb=, ts_keyframes=)")
        if device is not None:
            self.to(device)
        return self

    @torch.no_grad()
    def training_initialize(self, config=None, logger=None, log_prefix=None) -> bool:
        """No pre-training: the occupancy grid's ``init`` (constant, every slice fully occupied)."""
        self.accel.init()
        return False

    def _param_groups(self, cfg: dict):
        enc = self.encoding
        enc.shadow()
        groups = [dict(name="encoding", params=[enc.flattened_params], shadow16=lambda: enc.shadow()),
                  dict(name="dynamic_decoder", params=[self.den_w, self.den_b]),
                  dict(name="radiance_decoder", params=[self.rad_w, self.rad_b])]
        if self.use_flow:
            fenc = self.flow_encoding
            fenc.shadow()
            groups += [dict(name="flow_encoding", params=[fenc.flattened_params], shadow16=lambda: fenc.shadow()),
                       dict(name="flow_decoder", params=[self.flow_w, self.flow_b])]
        return groups

    def _after_optimizer_step(self):
        self._wpack_versions = None
        self._fwpack_versions = None

    def _weight_reg_tensors(self):
        return [self.den_w, self.rad_w] + ([self.flow_w] if self.use_flow else [])

    def set_active_levels(self, n: Optional[int]):
        """Hardmask over the lattice levels: levels >= n give zero features, get no gradient, and their tables are not read."""
        self.encoding.cfg.set_active_levels(n)
        self.meta.lotd.n_active_levels = self.encoding.cfg.meta.n_active_levels

    def _set_active_raw(self, n: int):
        self.meta.lotd.n_active_levels = n
        self.encoding.cfg.meta.n_active_levels = n
        self.encoding.cfg.pmeta.n_active_levels = n

    # ------------------------------------------------------------------ kernels' inputs
    def _shadow(self):
        """(fp16 table shadow, MFMA-fragment weight pack), refreshed lazily when a parameter changed in place."""
        grid16 = self.encoding.shadow()
        vers = (self.den_w._version, self.den_b._version, self.rad_w._version, self.rad_b._version, self.meta.precision,
                str(self.den_w.device), self.den_w.data_ptr())
        return grid16, self._weight_pack(
            "_wpack", vers, self.den_w.device, lambda: _lib.get_lib().nsim_dyn_wpack_bytes(self.meta),
            lambda buf: _lib.call("nsim_dyn_pack_weights", self.meta, _lib.ptr(self.den_w.detach()), _lib.ptr(self.den_b.detach()),
                                  _lib.ptr(self.rad_w.detach()), _lib.ptr(self.rad_b.detach()), _lib.ptr(buf)))

    def _flow_shadow(self):
        """(fp16 shadow of the flow table, weight pack of the flow decoder), refreshed lazily like ``_shadow``"""
        fgrid16 = self.flow_encoding.shadow()
        vers = (self.flow_w._version, self.flow_b._version, self.meta.precision, str(self.flow_w.device), self.flow_w.data_ptr())
        prec = int(self.meta.precision)
        return fgrid16, self._weight_pack(
            "_fwpack", vers, self.flow_w.device, lambda: _lib.get_lib().nsim_flow_wpack_bytes(prec),
            lambda buf: _lib.call("nsim_flow_pack_weights", int(self.flow_encoding.cfg.pmeta.num_levels), prec,
                                  _lib.ptr(self.flow_w.detach()), _lib.ptr(self.flow_b.detach()), _lib.ptr(buf)))

    def _query(self, h_appear, x4, rays_d, ridx, step, with_rgb, pose=(None, None, None, None)):
        """-> (sigma, alpha, rgb | None, flow dict | None): the plain decoder, or the flow-aggregated one with its four flow
        tensors ([S,3] each: the keys app/loss/flow.py reads).  ``pose`` = (x, rays_o, rays_d, t): the points or rays x4 was made
        of where they carry gradients."""
        if not self.use_flow:
            outs = _DynFn.apply(self, self.encoding.flattened_params, self.den_w, self.den_b, self.rad_w, self.rad_b, h_appear,
                                x4, rays_d, ridx, step, with_rgb, *pose)
            return outs[0], outs[1], (outs[2] if with_rgb else None), None
        outs = _DynFlowFn.apply(self, self.encoding.flattened_params, self.den_w, self.den_b, self.rad_w, self.rad_b, h_appear,
                                self.flow_encoding.flattened_params, self.flow_w, self.flow_b, x4, rays_d, ridx, step, with_rgb,
                                *pose)
        flow6, pred6 = outs[-2], outs[-1]
        S = x4.shape[0]
        flow = dict(flow_fwd=flow6[:, :3], flow_fwd_pred_bwd=pred6[:S, 3:], flow_bwd=flow6[:, 3:], flow_bwd_pred_fwd=pred6[S:, :3])
        return outs[0], outs[1], (outs[2] if with_rgb else None), flow

    def time_coord(self, ts: torch.Tensor) -> torch.Tensor:
        """w = SeqEmbedding(ts_keyframes, time_codes)(ts, 'interp'): the 4th lattice input of each time (no gradient)."""
        t = ts.detach().float().reshape(-1).contiguous()
        w = torch.empty([t.shape[0]], dtype=torch.float32, device=t.device)
        _lib.call("nsim_dyn_time", _lib.ptr(self.ts_keyframes), _lib.ptr(self.time_codes), int(self.ts_keyframes.shape[0]),
                  _lib.ptr(t), t.shape[0], 0, _lib.ptr(w), None, None)
        return w.reshape(ts.shape)

    def _points(self, w, S, x=None, rays=None):
        o, d, t, ridx = rays if rays is not None else (None, None, None, None)
        x4 = torch.empty([S, 4], dtype=torch.float32, device=w.device)
        _lib.call("nsim_dyn_points", _lib.ptr(x), _lib.ptr(o), _lib.ptr(d), _lib.ptr(t), _lib.ptr(ridx), _lib.ptr(w), S,
                  _lib.ptr(x4))
        return x4

    # ------------------------------------------------------------------ point queries
    def forward_density(self, x: torch.Tensor, ts: torch.Tensor, x_has_grad: bool = False) -> Dict[str, torch.Tensor]:
        """sigma at x [..., 3] (object coordinates) and times ts [...], with gradient to the table and the dynamic decoder -- and,
        with ``x_has_grad=True``, to x (pose refinement)."""
        if x.requires_grad and not x_has_grad:
            raise NotImplementedError("x.requires_grad: gradients to positions (pose refinement) are not built for this model "
                                      "unless asked for: forward_density(x, ts, x_has_grad=True)")
        if ts.requires_grad:
            raise NotImplementedError("ts.requires_grad: gradients to the time input are not built for this model")
        shape = x.shape[:-1]
        xf = x.detach().float().reshape(-1, 3).contiguous()
        S = xf.shape[0]
        if S == 0:
            ret = dict(sigma=torch.zeros(shape, dtype=torch.float32, device=xf.device))
            if self.use_flow:
                ret.update({k: torch.zeros([*shape, 3], dtype=torch.float32, device=xf.device) for k in FLOW_KEYS})
            return ret
        w = self.time_coord(ts.expand(shape).reshape(-1))
        x4 = self._points(w, S, x=xf)
        pose = (x.float().reshape(-1, 3), None, None, None) if x.requires_grad else (None,) * 4
        sigma, _, _, flow = self._query(None, x4, None, None, self._step(), False, pose)
        ret = dict(sigma=sigma.reshape(shape))
        if flow is not None:
            ret.update({k: v.reshape(*shape, 3) for k, v in flow.items()})
        return ret

    @torch.no_grad()
    def query_density(self, x: torch.Tensor, ts: torch.Tensor) -> torch.Tensor:
        return self.forward_density(x, ts)["sigma"]

    def sample_pts_uniform(self, num_pts: int, generator=None) -> Dict[str, torch.Tensor]:
        """Random points of the AABB at random keyframe times -> ``{'x', 'ts', 'sigma'}`` with gradient (and the four flow
        tensors of a with-flow model)."""
        lo, hi = self.accel.aabb[0], self.accel.aabb[1]
        x = lo + torch.rand([num_pts, 3], device=self.device, generator=generator) * (hi - lo)
        ts = self.ts_keyframes[torch.randint(int(self.ts_keyframes.shape[0]), [num_pts], device=self.device, generator=generator)]
        ret = self.forward_density(x, ts)
        ret["x"] = ret["net_x"] = x
        ret["ts"] = ts
        return ret

    # ------------------------------------------------------------------ rays
    def ray_test(self, rays_o, rays_d, near=None, far=None, rays_ts: torch.Tensor = None, **extra) -> Dict:
        """The AABB test; ``rays_ts`` [N] travels through the compaction with the other per-ray inputs."""
        if rays_ts is None:
            raise ValueError("rays_ts is missing: a time-conditioned model (use_ts) needs the time of every ray")
        if rays_ts.requires_grad:
            raise NotImplementedError("rays_ts.requires_grad: gradients to the time input are not built for this model")
        return aabb_ray_test(self.accel.aabb, self.accel.meta, rays_o, rays_d, near=near, far=far, rays_ts=rays_ts, **extra)

    def _check_rays(self, ray_tested, has_grad):
        if ray_tested.get("rays_ts", None) is None:
            raise ValueError("ray_tested['rays_ts'] is missing: a time-conditioned model (use_ts) needs the time of every ray")
        for k in ("rays_o", "rays_d", "rays_ts"):
            if ray_tested[k].requires_grad and not (has_grad and k != "rays_ts"):
                raise NotImplementedError(f"ray_tested[{k!r}].requires_grad: gradients to rays and times (pose refinement) are "
                                          f"not built for this model" + (" unless ray_query_cfg.query_param.rays_has_grad is set"
                                                                         if k != "rays_ts" else ""))

    def _march_extras(self, ray_tested):
        """The slice of each ray's time in the time-sliced accelerator, its word offset, and the rays' time coordinates."""
        ts = ray_tested["rays_ts"].detach().float().reshape(-1).contiguous()
        slices = torch.empty([ts.shape[0]], dtype=torch.long, device=ts.device)
        woff = torch.empty([ts.shape[0]], dtype=torch.long, device=ts.device)
        self.accel._time_call(ts, slices, woff)
        return woff, self.time_coord(ts), dict(slices=slices)

    def _decode(self, ray_tested, h_appear, o, d, t, ridx, w, step, with_rgb):
        x4 = self._points(w, t.shape[0], rays=(o, d, t, ridx))
        # (marching, the occupancy grid, the slice choice and the sample depths saw detached rays; the samples o + t d carry the graph)
        ro, rd = ray_tested["rays_o"], ray_tested["rays_d"]
        pose = (None, ro.float() if ro.requires_grad else None, rd.float() if rd.requires_grad else None, t) \
            if (ro.requires_grad or rd.requires_grad) else (None,) * 4
        sigma, alpha, rgb, flow = self._query(h_appear, x4, d, ridx, step, with_rgb, pose)
        return sigma, alpha, rgb, flow or {}

    def _collect(self, sigma, rays, extras):
        self.accel.collect(sigma, extras["slices"], rays=rays)
