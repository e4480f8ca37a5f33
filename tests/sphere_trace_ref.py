"""Restatement of the sphere tracer (``query_mode: sphere_trace``) in torch on the CPU, over the oracle's
SDF (``oracle.field.forward_sdf``) and the oracle's occupancy lattice (``oracle.render.voxel_index`` / ``march_lattice``).
TEST INFRASTRUCTURE: written from the three steps of the semantics, shares no code with neuralsim_amd/fields/sphere_trace.py.

Per ray, from t = near:
  1. voxel of o + t d unoccupied / outside -> t = the smallest occupied lattice point near + k step (jitter 0) that is > t;
     none -> OUT
  2. s = sdf(o + t d) (+ ``sdf_shift``), n_steps += 1; s <= hit_threshold -> HIT
  3. t += max(distance_scale s, min_step); t > far -> OUT; n_steps == max_march_iters -> ALIVE; else 1.
(t, sdf) of the result = the ray's last query; a ray that never queried keeps t = near and sdf = NaN."""
import torch

from oracle import field as ofield
from oracle import render as orr

ALIVE, HIT, OUT = 0, 1, 2


def trace(p, rays_o, rays_d, near, far, occ, aabb_min, aabb_max, res, *, step, max_steps, distance_scale, min_step,
          hit_threshold, max_march_iters, sdf_shift: float = 0.0):
    """-> dict(status u8 [R], n_steps i32 [R], t [R], sdf [R]) -- all float arithmetic in f32, one operation at a time."""
    R = rays_o.shape[0]
    res_t = torch.tensor(res, dtype=torch.long)
    scale = res_t.float() / (aabb_max - aabb_min)
    f32 = torch.float32
    t_occ, ridx, counts = orr.march_lattice(rays_o, rays_d, near, far, torch.zeros(R), occ.reshape(-1), aabb_min, scale, res_t,
                                            step, max_steps)
    # the occupied lattice points of every ray as a padded matrix [R, max count] (+inf behind the ray's own)
    C = int(counts.max()) if R else 0
    lat = torch.full([R, max(C, 1)], float("inf"), dtype=f32)
    start = torch.cumsum(counts, 0) - counts
    col = torch.arange(t_occ.shape[0]) - start[ridx]
    lat[ridx, col] = t_occ

    def occupied(x):
        flat, inside = orr.voxel_index(x, aabb_min, scale, res_t)
        return inside & occ.reshape(-1)[flat]

    def skip(idx, t):
        here = occupied(rays_o[idx] + t[:, None] * rays_d[idx])
        later = (lat[idx] > t[:, None]) & torch.isfinite(lat[idx])
        has = later.any(dim=1)
        nxt = lat[idx, later.float().argmax(dim=1)]
        return torch.where(here, t, nxt), here | has

    status = torch.full([R], ALIVE, dtype=torch.uint8)
    n_steps = torch.zeros([R], dtype=torch.int32)
    t = near.clone().to(f32)
    sdf = torch.full([R], float("nan"), dtype=f32)
    live = torch.arange(R)
    t0, found = skip(live, t)
    found &= near <= far
    status[~found] = OUT
    t[found] = t0[found]
    live = live[found]
    thr = torch.tensor(hit_threshold, dtype=f32)
    ds = torch.tensor(distance_scale, dtype=f32)
    ms = torch.tensor(min_step, dtype=f32)
    with torch.no_grad():
        while live.numel():
            s = ofield.forward_sdf(rays_o[live] + t[live][:, None] * rays_d[live], p).to(f32) + sdf_shift
            sdf[live] = s
            n_steps[live] += 1
            hit = s <= thr
            tn = t[live] + torch.maximum(ds * s, ms)
            out = ~hit & ~(tn <= far[live])
            stop = ~hit & ~out & (n_steps[live] >= max_march_iters)
            go = ~(hit | out | stop)
            status[live[hit]] = HIT
            status[live[out]] = OUT
            tg, found = skip(live[go], tn[go])
            status[live[go][~found]] = OUT
            nxt = live[go][found]
            t[nxt] = tg[found]
            live = nxt
    return dict(status=status, n_steps=n_steps, t=t, sdf=sdf)


def stable_rays(runs):
    """Rays whose ``status`` and ``n_steps`` agree in all the runs (SDF shifted by 0 and +-eps), and the per-ray spread of t."""
    st = torch.stack([r["status"] for r in runs])
    ns = torch.stack([r["n_steps"] for r in runs])
    tt = torch.stack([r["t"] for r in runs])
    stable = (st == st[0]).all(dim=0) & (ns == ns[0]).all(dim=0)
    return stable, tt.max(dim=0).values - tt.min(dim=0).values
