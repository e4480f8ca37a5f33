"""Sphere tracing of a trained SDF field: ``query_mode: sphere_trace`` of ``LoTDNeuSModel.ray_query`` and ``model.tracer``
(app/visualizer/gui_runner_single_cuboid.py:76-104, code_single/tools/inspect_rendering.py:71-73,98-109,262-287; the library's
csrc/sphere_trace extension is absent -- the semantics are fixed in DESIGN.md sec. 7).

Per ray, independently of every other ray, from ``t = near``:
  1. if the occupancy voxel of ``o + t d`` is unoccupied (or outside the grid), t moves to the smallest point of the march
     lattice ``near + k step_size`` (``march_cfg``, jitter 0) that is > t and lies in an occupied voxel; none: OUT;
  2. ``s = sdf(o + t d)``, ``n_steps += 1``; ``s <= hit_threshold``: HIT at this t;
  3. ``t += max(distance_scale s, min_step)``; ``t > far``: OUT; ``n_steps == max_march_iters``: ALIVE; else 1.

Two implementations of the same steps: ``trace_kernel`` -- one persistent launch (csrc/field.hip ``k_sphere_trace``) -- and
``trace_replay`` -- a host loop with one ``query_sdf`` launch and one advance step in torch per iteration, which also records
every iteration (``debug_replay`` of the reference's tracer).  Evaluation only: nothing here carries a gradient."""
from typing import Callable, Dict, Optional

import torch

from .. import _lib

ALIVE, HIT, OUT = 0, 1, 2
STATUS_NAMES = ["ALIVE", "HIT", "OUT"]           # inspect_rendering.py:285

# ``sphere_trace_cfg`` of inspect_rendering.py:71-73 / the presets of gui_runner_single_cuboid.py:76-104
PARAM_KEYS = ("distance_scale", "min_step", "hit_threshold", "max_march_iters", "drop_alive_rate", "tail_sample_threshold",
              "tail_sample_step_size", "debug", "march_cfg")
OBJECT_PRESET = dict(distance_scale=1.0, min_step=0.002, hit_threshold=1e-4, max_march_iters=500, drop_alive_rate=0.0,
                     tail_sample_threshold=20000, tail_sample_step_size=None)


def trace_params(qp: dict) -> dict:
    """``query_param`` of the mode -> the four numbers the tracer uses.  ``drop_alive_rate`` / ``tail_sample_*`` schedule the
    batches of the CUDA implementation: a non-default value of the two that would change results is refused by name (the
    convention of fields/ref_config.py), ``tail_sample_threshold`` is a hint without effect on results."""
    qp = dict(qp or {})
    unknown = sorted(set(qp) - set(PARAM_KEYS))
    if unknown:
        raise KeyError(f"query_mode='sphere_trace': unknown query_param keys {unknown}")
    if float(qp.get("drop_alive_rate", 0.0) or 0.0) != 0.0:
        raise NotImplementedError(f"query_mode='sphere_trace': query_param.drop_alive_rate = {qp['drop_alive_rate']!r} is not "
                                  f"implemented (only 0.: every ray is traced to its end)")
    if qp.get("tail_sample_step_size", None) is not None:
        raise NotImplementedError(f"query_mode='sphere_trace': query_param.tail_sample_step_size = "
                                  f"{qp['tail_sample_step_size']!r} is not implemented (only None)")
    p = dict(distance_scale=float(qp.get("distance_scale", OBJECT_PRESET["distance_scale"])),
             min_step=float(qp.get("min_step", OBJECT_PRESET["min_step"])),
             hit_threshold=float(qp.get("hit_threshold", OBJECT_PRESET["hit_threshold"])),
             max_march_iters=int(qp.get("max_march_iters", OBJECT_PRESET["max_march_iters"])))
    if p["max_march_iters"] < 1 or not p["min_step"] > 0:
        raise ValueError("query_mode='sphere_trace': max_march_iters >= 1 and min_step > 0 are required")
    return p


class SphereTracer:
    """``model.tracer`` (inspect_rendering.py:262-263)."""

    def __init__(self, model):
        self.model = model
        self.cfg = dict(OBJECT_PRESET)          # used by ``trace`` unless the model's ray_query_cfg is a sphere_trace one
        self.use_kernel = True                  # False: ``trace`` / the ray query run the host loop (profiles/sphere_trace.md)

    # ------------------------------------------------------------------ pieces
    def _march_cfg(self, qp: Optional[dict] = None):
        m = self.model
        march = (qp or {}).get("march_cfg") or dict(m.ray_query_cfg.get("query_param", {})).get("march_cfg") or {}
        return float(march.get("step_size", 0.005)), int(march.get("max_steps", 4096))

    def _query_param(self) -> dict:
        rq = self.model.ray_query_cfg
        return dict(rq.get("query_param", {})) if rq.get("query_mode") == "sphere_trace" else dict(self.cfg)

    @torch.no_grad()
    def query_sdf(self, x: torch.Tensor) -> torch.Tensor:
        """The SDF the tracer steps on: the model's no-grad query at the precision of its sampling pass
        (``NSIM_SAMPLING_PRECISION``; equal to ``model.query_sdf`` when that is the field's own precision)."""
        m = self.model
        shape = x.shape[:-1]
        x = x.detach().float().reshape(-1, 3).contiguous()
        fm, wpack = m._sampling_ctx()
        return m._sdf_query(m._table16(), wpack, x, None, None, None, None, x.shape[0], x.device, fm=fm).reshape(shape)

    @staticmethod
    def _rays(ray_tested: dict):
        o = ray_tested["rays_o"].detach().float().contiguous()
        d = ray_tested["rays_d"].detach().float().contiguous()
        return o, d, ray_tested["near"].detach().float().contiguous(), ray_tested["far"].detach().float().contiguous()

    # ------------------------------------------------------------------ the persistent kernel
    @torch.no_grad()
    def trace_kernel(self, o, d, near, far, prm: dict, march=None) -> Dict[str, torch.Tensor]:
        """-> dict(status u8 [R], n_steps i32 [R], t [R], sdf [R]); (t, sdf) = the ray's last query (NaN sdf: none)."""
        m = self.model
        if m.plane_levels != 16 or m.pos_embed_E:
            raise NotImplementedError("query_mode='sphere_trace': the tracer kernel exists for pyramids of <= 16 levels "
                                      "without an embedded-position block")
        R, dev = o.shape[0], o.device
        step, max_steps = march if march is not None else self._march_cfg()
        out = dict(status=torch.empty([R], dtype=torch.uint8, device=dev), n_steps=torch.empty([R], dtype=torch.int32, device=dev),
                   t=torch.empty([R], dtype=torch.float32, device=dev), sdf=torch.empty([R], dtype=torch.float32, device=dev))
        if R == 0:
            return out
        fm, wpack = m._sampling_ctx()
        ws = torch.empty([int(_lib.get_lib().nsim_sphere_trace_workspace_bytes())], dtype=torch.uint8, device=dev)
        _lib.call("nsim_sphere_trace", fm, _lib.ptr(m._table16()), _lib.ptr(wpack), _lib.ptr(o), _lib.ptr(d), _lib.ptr(near),
                  _lib.ptr(far), R, _lib.ptr(m.accel.occ_bits), m.accel.meta, step, max_steps, prm["distance_scale"],
                  prm["min_step"], prm["hit_threshold"], prm["max_march_iters"], _lib.ptr(out["t"]), _lib.ptr(out["sdf"]),
                  _lib.ptr(out["status"]), _lib.ptr(out["n_steps"]), _lib.ptr(ws))
        return out

    # ------------------------------------------------------------------ the host loop
    def _occupied_lattice(self, o, d, near, far, march):
        """(t_m [M], pack infos [R, 2]) of the occupied march-lattice points of every ray (nsim_march_*, jitter 0)."""
        from ..graphics import pack_ops as po
        m = self.model
        R, dev = o.shape[0], o.device
        step, max_steps = march
        jit = torch.zeros([R], dtype=torch.float32, device=dev)
        counts = torch.empty([R], dtype=torch.long, device=dev)
        bits, occm = m.accel.occ_bits, m.accel.meta
        _lib.call("nsim_march_count", _lib.ptr(o), _lib.ptr(d), _lib.ptr(near), _lib.ptr(far), _lib.ptr(jit), R, _lib.ptr(bits),
                  None, occm, step, max_steps, _lib.ptr(counts))
        pi = po.get_pack_infos_from_n(counts)
        M = int(counts.sum().item())
        t_m = torch.empty([max(M, 1)], dtype=torch.float32, device=dev)
        if M:
            _lib.call("nsim_march_emit", _lib.ptr(o), _lib.ptr(d), _lib.ptr(near), _lib.ptr(far), _lib.ptr(jit), R, _lib.ptr(bits),
                      None, occm, step, max_steps, _lib.ptr(pi), _lib.ptr(t_m))
        else:
            t_m.zero_()
        return t_m, pi

    def _voxel_occupied(self, x):
        acc = self.model.accel
        lo = acc.aabb[0]
        res = torch.tensor(acc.resolution, dtype=torch.float32, device=x.device)
        scale = torch.tensor([acc.meta.scale[i] for i in range(3)], dtype=torch.float32, device=x.device)
        g = torch.floor((x - lo) * scale)
        inside = ((g >= 0) & (g < res)).all(dim=-1)
        gi = g.clamp_min(0).minimum(res - 1).long()
        flat = gi[:, 0] + acc.resolution[0] * (gi[:, 1] + acc.resolution[1] * gi[:, 2])
        word = acc.occ_bits[flat >> 5].long()
        return inside & (((word >> (flat & 31)) & 1) != 0)

    @staticmethod
    def _next_lattice(t, t_m, lo, hi):
        """Per ray: index of the first entry of its pack [lo, hi) of t_m that is > t (hi: none) -- a bisection in torch."""
        lo, hi = lo.clone(), hi.clone()
        last = t_m.shape[0] - 1
        for _ in range(max(int(hi.sub(lo).max().item()), 1).bit_length()):
            mid = (lo + hi) >> 1
            open_ = lo < hi
            right = open_ & (t_m[mid.clamp(max=last)] <= t)
            lo = torch.where(right, mid + 1, lo)
            hi = torch.where(open_ & ~right, mid, hi)
        return lo

    @torch.no_grad()
    def trace_replay(self, o, d, near, far, prm: dict, sdf_fn: Optional[Callable] = None, debug_output: Optional[dict] = None,
                     march=None, print_debug_log: bool = False) -> Dict[str, torch.Tensor]:
        """The same steps as ``trace_kernel`` as a host loop: per iteration one SDF launch on the live rays (``sdf_fn``, default
        ``self.query_sdf``) and one advance step in torch.  ``debug_output``: filled with ``segs`` -- the occupied [t0, t1] runs of
        ray 0 on the march lattice -- and ``trace_data`` -- per iteration ``rays_alive{t, n_steps, status}`` and ``d`` (the SDFs) of
        the rays queried in it (inspect_rendering.py:266-287)."""
        sdf_fn = self.query_sdf if sdf_fn is None else sdf_fn
        R, dev = o.shape[0], o.device
        march = march if march is not None else self._march_cfg()
        status = torch.full([R], ALIVE, dtype=torch.uint8, device=dev)
        n_steps = torch.zeros([R], dtype=torch.int32, device=dev)
        t = near.clone()
        sdf = torch.full([R], float("nan"), dtype=torch.float32, device=dev)
        out = dict(status=status, n_steps=n_steps, t=t, sdf=sdf)
        if R == 0:
            return out
        t_m, pi = self._occupied_lattice(o, d, near, far, march)
        seg_lo, seg_hi = pi[:, 0], pi[:, 0] + pi[:, 1]
        if debug_output is not None:
            debug_output["segs"] = self._segments(t_m[int(seg_lo[0]):int(seg_hi[0])], march[0])
            debug_output["trace_data"] = []

        def skip(idx, t_new):
            """step 1 for the rays ``idx`` at depths ``t_new`` -> (depths, found)"""
            occ = self._voxel_occupied(o[idx] + t_new[:, None] * d[idx])
            k = self._next_lattice(t_new, t_m, seg_lo[idx], seg_hi[idx])
            has = k < seg_hi[idx]
            return torch.where(occ, t_new, t_m[k.clamp(max=t_m.shape[0] - 1)]), occ | has
        live = torch.arange(R, device=dev)
        ok = near <= far
        t0, found = skip(live, t)
        found &= ok
        t[found] = t0[found]
        status[~found] = OUT
        live = live[found]
        it = 0
        while live.numel():
            x = o[live] + t[live][:, None] * d[live]
            s = sdf_fn(x)
            s = (s["sdf"] if isinstance(s, dict) else s).detach().float().reshape(-1)
            sdf[live] = s
            n_steps[live] += 1
            hit = s <= prm["hit_threshold"]
            t_new = t[live] + torch.clamp_min(prm["distance_scale"] * s, prm["min_step"])
            out_ = ~hit & ~(t_new <= far[live])
            alive_end = ~hit & ~out_ & (n_steps[live] >= prm["max_march_iters"])
            go = ~hit & ~out_ & ~alive_end
            t_go, found = skip(live[go], t_new[go])
            st = torch.full_like(s, ALIVE, dtype=torch.uint8)
            st[hit] = HIT
            st[out_] = OUT
            go_idx = go.nonzero()[:, 0]
            st[go_idx[~found]] = OUT
            status[live] = st
            if debug_output is not None:
                debug_output["trace_data"].append(dict(rays_alive=dict(t=t[live].clone(), n_steps=n_steps[live].clone(), status=st.clone(),
                                                                       rays_inds=live.clone()), d=s.clone()))
            nxt = live[go][found]
            t[nxt] = t_go[found]
            live = nxt
            it += 1
            if print_debug_log:
                print(f"[sphere_trace] iter {it}: {int(hit.sum())} hit, {int(out_.sum()) + int((~found).sum())} out, "
                      f"{int(alive_end.sum())} stopped, {live.numel()} alive")
        return out

    @staticmethod
    def _segments(t_occ: torch.Tensor, step: float) -> torch.Tensor:
        """Occupied lattice depths of one ray -> [n, 2] runs [t0, t1] of consecutive lattice points (t1 = last point + step)."""
        if t_occ.numel() == 0:
            return t_occ.new_zeros([0, 2])
        brk = (t_occ[1:] - t_occ[:-1]) > 1.5 * step
        first = torch.cat([brk.new_ones([1]), brk])
        last = torch.cat([brk, brk.new_ones([1])])
        return torch.stack([t_occ[first], t_occ[last] + step], dim=-1)

    # ------------------------------------------------------------------ the reference's entry point
    @torch.no_grad()
    def trace(self, ray_tested: dict, sdf_fn: Optional[Callable] = None, print_debug_log: bool = False,
              debug_output: Optional[dict] = None, debug_replay: bool = False, query_param: Optional[dict] = None) -> dict:
        """``obj.model.tracer.trace(ray_tested, sdf_fn, print_debug_log=, debug_output=, debug_replay=)`` -> the hit rays:
        dict(rays_inds_hit, idx (rows of ``ray_tested``), t, sdf, num_rays_hit) + ``details`` (status, n_steps, t, sdf of every
        tested ray).  ``debug_replay``: the host loop, on ``sdf_fn`` (a callable on points [n, 3] returning the SDF or a dict
        with it, e.g. ``model.forward_sdf``; None: ``self.query_sdf``), recording into ``debug_output``.  Otherwise the
        persistent kernel, which steps on ``self.query_sdf``'s values."""
        qp = dict(self._query_param() if query_param is None else query_param)
        prm = trace_params(qp)
        march = self._march_cfg(qp)
        o, d, near, far = self._rays(ray_tested)
        if debug_replay or not self.use_kernel:
            res = self.trace_replay(o, d, near, far, prm, sdf_fn=sdf_fn if debug_replay else None,
                                    debug_output=debug_output if debug_replay else None, march=march,
                                    print_debug_log=print_debug_log)
        else:
            res = self.trace_kernel(o, d, near, far, prm, march=march)
        idx = (res["status"] == HIT).nonzero()[:, 0]
        if print_debug_log:
            n = res["n_steps"].float()
            print(f"[sphere_trace] {o.shape[0]} rays: {idx.numel()} hit, {int((res['status'] == OUT).sum())} out, "
                  f"{int((res['status'] == ALIVE).sum())} alive; n_steps mean {float(n.mean()) if n.numel() else 0:.2f} "
                  f"max {int(n.max()) if n.numel() else 0}")
        return dict(rays_inds_hit=ray_tested["rays_inds"][idx], idx=idx, t=res["t"][idx], sdf=res["sdf"][idx],
                    num_rays_hit=int(idx.numel()), details=res)
