"""float64 statements of the pose-refinement gradients (rays or points that carry gradients) the kernels of csrc/nerf_field.hip are
checked against in tests/test_pose_grad.py: the position gradient of the level-major LoTD gather (``nsim_lotd_dx_lm``) as autograd
through ``oracle.lotd.lotd_forward``, the ray / point gradients of ``LoTDNeRFModel`` as autograd through ``nerf_ref.query_at``, and
those of the EmerNeRF dynamic model through ``dynamic_nerf_ref`` / ``dynamic_flow_ref`` (with an fp16 rounding hook for the probe
behind the one fp16 bound that is this file's).  Also the near-face exclusion rule of those tests.  Test infrastructure only."""
import copy

import torch

import nerf_ref as nr
from oracle import lotd as ol

MIN_GAP = 1e-4              # lattice units: a sample closer than this to a cell face on an active level is left out
MAX_EXCLUDED_SAMPLES = 0.02
MAX_EXCLUDED_RAYS = 0.10


def face_gap(x: torch.Tensor, spec: ol.LoTDSpec, n_active: int = None) -> torch.Tensor:
    """x [S,3] -> [S] the smallest distance, in lattice units over the active levels and the three axes, to a cell face (where the
    position gradient of the piecewise-trilinear interpolant jumps)."""
    u = spec.unit_coords(x.double())
    L = spec.num_levels if n_active is None else min(n_active, spec.num_levels)
    gap = torch.full([x.shape[0]], float("inf"), dtype=torch.float64)
    for R in spec.lod_res[:L]:
        pos = u * (torch.tensor(ol._res3(R), dtype=torch.float64) - 1.0)
        gap = torch.minimum(gap, (pos - torch.round(pos)).abs().min(dim=-1).values)
    return gap


def lotd_dx(x: torch.Tensor, table: torch.Tensor, spec: ol.LoTDSpec, dh: torch.Tensor, n_active: int = None) -> torch.Tensor:
    """d (dh . h(x)) / d x in float64: x [S,3] object coordinates, dh [S, 2 L]."""
    xd = x.double().clone().requires_grad_(True)
    h = ol.lotd_forward(xd, table.double(), spec, n_active=n_active)
    (h * dh.double()).sum().backward()
    return xd.grad


def short_rays(S: int, seed: int, aabb: torch.Tensor, step: float, d_norm=(0.5, 2.0), empty_ray: bool = True, cyc=(4, 3, 2, 4, 1, 3)):
    """Rays with at most 4 samples each, S samples in all: origins in the middle of the box, un-normalised directions with norms in
    ``d_norm``, t = near + k step.  -> dict(o, d [R,3], near, far [R], counts [R], t, ridx [S]); ``far`` = near + (count - 1/2) step is
    what makes a lattice marcher over a fully occupied grid emit exactly these samples.  ``empty_ray``: ray 1 has no sample.
    ``cyc``: the samples per ray, cycled."""
    g = torch.Generator().manual_seed(seed)
    counts = []
    while sum(counts) < S:
        if empty_ray and len(counts) == 1:
            counts.append(0)
            continue
        counts.append(min(cyc[len(counts) % len(cyc)], S - sum(counts)))
    if empty_ray and len(counts) == 1:
        counts.append(0)
    counts = torch.tensor(counts)
    R = counts.shape[0]
    lo, hi = aabb[0], aabb[1]
    ext = hi - lo
    o = lo + ext * (0.4 + 0.2 * torch.rand(R, 3, generator=g))
    d = torch.randn(R, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True) * (d_norm[0] + (d_norm[1] - d_norm[0]) * torch.rand(R, 1, generator=g))
    near = 0.02 + 0.03 * torch.rand(R, generator=g)
    far = near + (counts.float() - 0.5) * step
    ridx = torch.repeat_interleave(torch.arange(R), counts)
    k = torch.cat([torch.arange(int(c)) for c in counts]).float() if S else torch.zeros(0)
    t = near[ridx] + k * step
    x = o[ridx] + t[:, None] * d[ridx]
    assert bool(((x > lo + 0.02 * ext) & (x < hi - 0.02 * ext)).all()), "the samples stay inside the box"
    return dict(o=o, d=d, near=near, far=far, counts=counts, t=t, ridx=ridx)


def excluded(r: dict, spec: ol.LoTDSpec, n_active: int = None):
    """-> (samples [S] bool, rays [R] bool): the samples within MIN_GAP of a face -- at the float64 position of the f32 ray data and at
    its f32 rounding, the position a kernel given points sees -- and the rays that own one."""
    x64 = r["o"].double()[r["ridx"]] + r["t"].double()[:, None] * r["d"].double()[r["ridx"]]
    x32 = (r["o"][r["ridx"]] + r["t"][:, None] * r["d"][r["ridx"]])
    ex = (face_gap(x64, spec, n_active) < MIN_GAP) | (face_gap(x32, spec, n_active) < MIN_GAP)
    rays = torch.zeros(r["o"].shape[0], dtype=torch.bool)
    rays[r["ridx"][ex]] = True
    return ex, rays


def pick_rays(S: int, spec: ol.LoTDSpec, aabb: torch.Tensor, step: float, n_active: int = None, base_seed: int = 0, **kw):
    """The first seed (from ``base_seed``) whose rays meet both exclusion caps, by this file alone.  -> (seed, rays, ex_s, ex_r)"""
    for seed in range(base_seed, base_seed + 64):
        r = short_rays(S, seed, aabb, step, **kw)
        ex_s, ex_r = excluded(r, spec, n_active)
        if float(ex_s.float().mean()) <= MAX_EXCLUDED_SAMPLES and float(ex_r.float().mean()) <= MAX_EXCLUDED_RAYS:
            return seed, r, ex_s, ex_r
    raise AssertionError("no seed meets the exclusion caps: shorten the rays")


def to_double(p: nr.NerfParams) -> nr.NerfParams:
    q = copy.copy(p)
    q.spec = copy.copy(p.spec)
    q.grid = p.grid.detach().double()
    for k in ("den_w", "den_b", "rad_w", "rad_b"):
        setattr(q, k, [w.detach().double() for w in getattr(p, k)])
    q.aabb = p.aabb.double()
    return q


def ngp_ray_grads(p: nr.NerfParams, r: dict, step: float, cot: dict, h_appear=None, with_rgb=True, rounding=None):
    """Autograd of sum(sigma ws) + sum(alpha wa) [+ sum(rgb wr)] through ``nerf_ref.query_at`` in float64.
    -> dict(o, d: ray gradients; sigma, alpha, rgb: values; params: the NerfParams whose tensors hold their gradients)."""
    q = to_double(p).requires_grad_(True)
    o = r["o"].double().clone().requires_grad_(True)
    d = r["d"].double().clone().requires_grad_(True)
    ha = h_appear.double() if h_appear is not None else None
    out = nr.query_at(q, o, d, r["t"].double(), r["ridx"], step, ha, with_rgb=with_rgb, rounding=rounding)
    loss = (out["sigma"] * cot["ws"].double()).sum() + (out["opacity_alpha"] * cot["wa"].double()).sum()
    if with_rgb:
        loss = loss + (out["rgb"] * cot["wr"].double()).sum()
    loss.backward()
    return dict(o=o.grad, d=d.grad, sigma=out["sigma"].detach(), alpha=out["opacity_alpha"].detach(),
                rgb=out["rgb"].detach() if with_rgb else None, params=q)


def ngp_point_grads(p: nr.NerfParams, x: torch.Tensor, ws: torch.Tensor):
    """d sum(sigma ws) / d x through ``nerf_ref.density`` in float64."""
    q = to_double(p)
    xd = x.double().clone().requires_grad_(True)
    sigma, _, _ = nr.density(q, xd)
    (sigma * ws.double()).sum().backward()
    return xd.grad, sigma.detach()


def round16(v: torch.Tensor) -> torch.Tensor:
    """the fp16 rounding probe's ``rounding`` hook (straight-through: the rounding itself has no derivative)"""
    return v + (v.detach().half().to(v.dtype) - v.detach())


# ------------------------------------------------------------------------------------------------ the dynamic model
import dynamic_flow_ref as fref      # noqa: E402
import dynamic_nerf_ref as dr        # noqa: E402


def lattice_gap(spec, aabb, x, w) -> torch.Tensor:
    """[S]: the smallest barycentric weight over the levels of a 4-D lattice at (AABB-normalised x, w) -- 0 is a simplex face"""
    a = torch.as_tensor(aabb, dtype=torch.float64)
    c, h = (a[0] + a[1]) * 0.5, (a[1] - a[0]) * 0.5
    return fref.face_gap(torch.cat([(x.double() - c) / h, w.double().reshape(-1, 1)], dim=-1), spec)


def dyn_rays(S: int, seed: int, T: int, aabb, step: float, **kw) -> dict:
    """``short_rays`` with a time per ray: the first and the last keyframe (both clamps of w+-), a midpoint, an off-grid value"""
    r = short_rays(S, seed, torch.as_tensor(aabb, dtype=torch.float32), step, **kw)
    kf = torch.arange(T, dtype=torch.float32) * 0.25
    cand = torch.stack([kf[0], kf[-1], (kf[0] + kf[-1]) * 0.5, kf[0] + 0.0625])
    r["ts"] = cand[torch.arange(r["o"].shape[0]) % 4]
    return r


def dyn_sample_gap(p, fp, x64, x32, ts_s) -> torch.Tensor:
    """[S]: the smallest barycentric weight a sample meets -- the dynamic lattice at the sample (float64 and f32 position) and, with
    flow, the flow lattice there and both lattices at the two flow-warped points of the restatement"""
    x64, x32 = x64.double(), x32.double()
    w = dr.time_coord(p.ts_keyframes, p.codes, ts_s)
    gap = torch.minimum(lattice_gap(p.spec, p.aabb, x64, w), lattice_gap(p.spec, p.aabb, x32, w))
    if fp is not None:
        T = int(p.codes.shape[0])
        _, wp, wm = fref.time_neighbours(w, T, -1.0, 1.0)
        with torch.no_grad():
            f6 = fref.flow_at(fp, p.aabb, x64, w)
        for spec in (p.spec, fp.spec):
            for xx, ww in ((x64, w), (x32, w), (x64 + f6[:, :3], wp), (x64 + f6[:, 3:], wm)):
                gap = torch.minimum(gap, lattice_gap(spec, p.aabb, xx, ww))
    return gap


def dyn_excluded(p, fp, r: dict):
    """-> (samples [S] bool, rays [R] bool) within MIN_GAP of a simplex face (``dyn_sample_gap``)"""
    ridx = r["ridx"]
    x64 = r["o"].double()[ridx] + r["t"].double()[:, None] * r["d"].double()[ridx]
    x32 = (r["o"][ridx] + r["t"][:, None] * r["d"][ridx]).double()
    w = dr.time_coord(p.ts_keyframes, p.codes, r["ts"][ridx])
    gap = torch.minimum(lattice_gap(p.spec, p.aabb, x64, w), lattice_gap(p.spec, p.aabb, x32, w))
    if fp is not None:
        T = int(p.codes.shape[0])
        _, wp, wm = fref.time_neighbours(w, T, -1.0, 1.0)
        with torch.no_grad():
            f6 = fref.flow_at(fp, p.aabb, x64, w)
        for spec in (p.spec, fp.spec):
            for xx, ww in ((x64, w), (x32, w), (x64 + f6[:, :3], wp), (x64 + f6[:, 3:], wm)):
                gap = torch.minimum(gap, lattice_gap(spec, p.aabb, xx, ww))
    ex = gap < MIN_GAP
    rays = torch.zeros(r["o"].shape[0], dtype=torch.bool)
    rays[ridx[ex]] = True
    return ex, rays


def pick_dyn_rays(S: int, p, fp, step: float, base_seed: int = 0, per_sample: bool = True, **kw):
    """the first seed whose rays meet the exclusion caps, by this file alone -> (seed, rays, ex_s, ex_r).  ``per_sample`` False: a
    test that compares per ray only -- the cap on the rays alone."""
    for seed in range(base_seed, base_seed + 64):
        r = dyn_rays(S, seed, int(p.codes.shape[0]), p.aabb, step, **kw)
        ex_s, ex_r = dyn_excluded(p, fp, r)
        if (not per_sample or float(ex_s.float().mean()) <= MAX_EXCLUDED_SAMPLES) and float(ex_r.float().mean()) <= MAX_EXCLUDED_RAYS:
            return seed, r, ex_s, ex_r
    raise AssertionError("no seed meets the exclusion caps: shorten the rays")


def _leaf_copy(obj, names):
    q = copy.copy(obj)
    for k in names:
        v = getattr(obj, k)
        setattr(q, k, [t.detach().clone().requires_grad_(True) for t in v] if isinstance(v, list)
                else v.detach().clone().requires_grad_(True))
    return q


def dyn_query_rounded(p, fp, x, ts, view_dirs, h_appear, step, rounding):
    """``dynamic_nerf_ref.query_points`` / ``dynamic_flow_ref.query_points`` with the ``rounding`` hook of ``nerf_ref.density`` /
    ``nerf_ref.radiance``: applied to the weights and to every layer's input (the fp16 rounding probe; biases, lattice features'
    interpolation and activations stay float64).  ``rounding=None`` is the restatement itself."""
    rd = rounding or (lambda v: v)
    w = dr.time_coord(p.ts_keyframes, p.codes, ts)
    x = x.double()

    def feats(spec, grid, xx, ww, n_active=None):
        return fref._lattice(spec, grid, p.aabb, xx, ww, n_active)

    def hidden(xx, ww):
        return torch.relu(rd(feats(p.spec, p.grid, xx, ww, p.n_active)) @ rd(p.den_w[0]).t() + p.den_b[0])
    out = {}
    if fp is None:
        a = hidden(x, w)
    else:
        T = int(p.codes.shape[0])
        _, wp, wm = fref.time_neighbours(w, T, -1.0, 1.0)
        F = fp.spec.out_features
        w1, w2, w3 = fp.w[:64 * F].view(64, F), fp.w[64 * F:64 * F + 4096].view(64, 64), fp.w[64 * F + 4096:].view(6, 64)
        b1, b2, b3 = fp.b[:64], fp.b[64:128], fp.b[128:]

        def flow(xx, ww):
            a1 = torch.relu(rd(feats(fp.spec, fp.grid, xx, ww)) @ rd(w1).t() + b1)
            a2 = torch.relu(rd(a1) @ rd(w2).t() + b2)
            return rd(a2) @ rd(w3).t() + b3
        f6 = flow(x, w)
        xp, xm = x + f6[:, :3], x + f6[:, 3:]
        pp, pm = flow(xp, wp), flow(xm, wm)
        a = 0.5 * hidden(x, w) + 0.25 * hidden(xp, wp) + 0.25 * hidden(xm, wm)
        out.update(flow_fwd=f6[:, :3], flow_fwd_pred_bwd=pp[:, 3:], flow_bwd=f6[:, 3:], flow_bwd_pred_fwd=pm[:, :3])
    o2 = rd(a) @ rd(p.den_w[1]).t() + p.den_b[1]
    sigma = dr.trunc_softplus(o2[:, 0])
    out.update(sigma=sigma, opacity_alpha=1.0 - torch.exp(-sigma * step))
    if view_dirs is not None:
        v = view_dirs.double()
        inp = [o2[:, 1:], dr.sh4(v / v.norm(dim=-1, keepdim=True))]
        if p.n_appear:
            inp.append(h_appear.double())
        rr = torch.cat(inp, dim=-1)
        rr = torch.relu(rd(rr) @ rd(p.rad_w[0]).t() + p.rad_b[0])
        rr = torch.relu(rd(rr) @ rd(p.rad_w[1]).t() + p.rad_b[1])
        out["rgb"] = torch.sigmoid(rd(rr) @ rd(p.rad_w[2]).t() + p.rad_b[2])
    return out


def dyn_ray_grads(p, fp, r: dict, step: float, cot: dict, h_appear=None, with_rgb=True, flow_weights=None, rounding=None):
    """Autograd in float64 of sum(sigma ws) + sum(alpha wa) [+ sum(rgb wr)] [+ the cycle and sparsity terms of the flow loss] through
    ``dynamic_nerf_ref.query_at`` (fp None) or ``dynamic_flow_ref.query_points``, with respect to the rays and every parameter.
    -> dict(o, d, the values, params = (DynParams, FlowParams | None) holding their gradients)"""
    q = _leaf_copy(p, ("grid", "den_w", "den_b", "rad_w", "rad_b"))
    fq = _leaf_copy(fp, ("grid", "w", "b")) if fp is not None else None
    o = r["o"].double().clone().requires_grad_(True)
    d = r["d"].double().clone().requires_grad_(True)
    ridx, ts = r["ridx"], r["ts"].double()
    ha = h_appear.double() if (h_appear is not None and p.n_appear) else None
    if rounding is not None:
        x = o[ridx] + r["t"].double()[:, None] * d[ridx]
        out = dyn_query_rounded(q, fq, x, ts[ridx], d[ridx] if with_rgb else None, ha[ridx] if (ha is not None and with_rgb) else None,
                                step, rounding)
    elif fp is None:
        out = dr.query_at(q, o, d, ts, r["t"], ridx, step, ha, with_rgb=with_rgb)
    else:
        x = o[ridx] + r["t"].double()[:, None] * d[ridx]
        out = fref.query_points(q, fq, x, ts[ridx], d[ridx] if with_rgb else None,
                                ha[ridx] if (ha is not None and with_rgb) else None, step)
    loss = (out["sigma"] * cot["ws"].double()).sum() + (out["opacity_alpha"] * cot["wa"].double()).sum()
    if with_rgb:
        loss = loss + (out["rgb"] * cot["wr"].double()).sum()
    if fp is not None and flow_weights is not None:
        cyc, spa = fref.flow_loss(*[out[k] for k in fref.FLOW_KEYS], w_cycle=flow_weights[0], w_sparsity=flow_weights[1])
        loss = loss + cyc + spa
    loss.backward()
    ret = {k: v.detach() for k, v in out.items()}
    ret.update(o=o.grad, d=d.grad, params=(q, fq))
    return ret


# ------------------------------------------------------------------------------------------------ compose: street + dynamic object
def field_to_double(p):
    """oracle.field.FieldParams in float64"""
    q = copy.copy(p)
    q.grid = p.grid.detach().double()
    for k in ("sdf_w", "sdf_b", "rad_w", "rad_b"):
        setattr(q, k, [w.detach().double() for w in getattr(p, k)])
    q.ln_inv_s = p.ln_inv_s.detach().double()
    return q


def _buffer_samples(vb, o, d):
    """(ray of each sample, sample positions) of a packed per-object buffer: x = o[ray] + t d[ray], t the buffer's own depths"""
    from oracle import pack_ops as opo
    t = vb["t"].detach().cpu()
    ray = vb["rays_inds_hit"].cpu()[opo.pack_ridx(vb["pack_infos_hit"].cpu(), t.shape[0])]
    return ray, t, o[ray] + t.to(o.dtype)[:, None] * d[ray]


def compose_excluded(street_p, dyn_p, dyn_fp, vb_street, vb_dyn, o, d, ts):
    """[N] bool: the rays that own a sample -- of either object's buffer -- within MIN_GAP of a face of a lattice it meets"""
    bad = torch.zeros(o.shape[0], dtype=torch.bool)
    ray, _, x64 = _buffer_samples(vb_street, o.double(), d.double())
    _, _, x32 = _buffer_samples(vb_street, o, d)
    bad[ray[(face_gap(x64, street_p.spec) < MIN_GAP) | (face_gap(x32, street_p.spec) < MIN_GAP)]] = True
    ray, _, x64 = _buffer_samples(vb_dyn, o.double(), d.double())
    _, _, x32 = _buffer_samples(vb_dyn, o, d)
    bad[ray[dyn_sample_gap(dyn_p, dyn_fp, x64, x32, ts[ray]) < MIN_GAP]] = True
    return bad


def compose_ray_grads(street_p, dyn_p, dyn_fp, vb_street, vb_dyn, o, d, ts, ha, gt, dyn_step: float):
    """d mean((rgb_volume - gt)^2) / d (rays_o, rays_d) of the scene a NeuS street + the dynamic object, in float64, at the sample
    depths of the two per-object buffers (constants of the step): the street through ``oracle.field.forward_field`` and the NeuS
    alpha of its packs, the object through this file's query, both merged ray by ray in depth order and composited
    (``oracle.render.compose_buffers``).  -> (d_o [N,3], d_d [N,3], rgb_volume [N,3])"""
    from oracle import field as ofield, render as orr
    N = o.shape[0]
    o64, d64 = o.double().clone().requires_grad_(True), d.double().clone().requires_grad_(True)
    ha64 = ha.double()
    sp = field_to_double(street_p)
    ray, t, x = _buffer_samples(vb_street, o64, d64)
    sdf, _, rgb = ofield.forward_field(x, d64[ray], ha64[ray], sp, x_has_grad=True)
    pi_s = vb_street["pack_infos_hit"].cpu()
    bufs = [dict(rays_inds=vb_street["rays_inds_hit"].cpu(), pack_infos=pi_s, t=t.double(),
                 alpha=orr.neus_alpha_packed(sdf, pi_s, sp.inv_s()), rgb=rgb)]
    ray, t, x = _buffer_samples(vb_dyn, o64, d64)
    out = dyn_query_rounded(dyn_p, dyn_fp, x, ts.double()[ray], d64[ray], ha64[ray] if dyn_p.n_appear else None, dyn_step, None)
    bufs.append(dict(rays_inds=vb_dyn["rays_inds_hit"].cpu(), pack_infos=vb_dyn["pack_infos_hit"].cpu(), t=t.double(),
                     alpha=out["opacity_alpha"], rgb=out["rgb"]))
    _, _, rgb_vol, _ = orr.compose_buffers(bufs, N)
    ((rgb_vol.double() - gt.double()) ** 2).mean().backward()
    return o64.grad, d64.grad, rgb_vol.detach()


def dyn_point_grads(p, fp, x, ts, ws):
    """d sum(sigma ws) / d x at points x [S,3] with times ts [S], float64"""
    xd = x.double().clone().requires_grad_(True)
    out = dr.query_points(p, xd, ts.double()) if fp is None else fref.query_points(p, fp, xd, ts.double())
    (out["sigma"] * ws.double()).sum().backward()
    return xd.grad, out["sigma"].detach()


def flow_rounding_probe(shapes, step, flow_weights, rays_kw, cot_of, seeds=(11, 12, 13)):
    """What fp16 rounding alone costs on the ray gradients of the with-flow model: {(shape, model seed): (rel-L2 rays_o, rays_d)}
    of the rounded restatement against the unrounded one, on the rays the test of that shape uses for that model."""
    from util import rel_l2
    out = {}
    for S, T, na, Ld, Lf in shapes:
        for ms in seeds:
            p = dr.make_dyn_params(torch.arange(T, dtype=torch.float32) * 0.25, torch.tensor([[-2.0, -1, -1], [2.0, 1, 1]]), Ld, 10, 4.0,
                                   32.0, na, seed=ms)
            fp = fref.make_flow_params(Lf, 10, seed=ms + 6)
            seed, r, _, ex_r = pick_dyn_rays(S, p, fp, step, **rays_kw)
            ha = torch.randn(r["o"].shape[0], 4, generator=torch.Generator().manual_seed(seed)) * 0.3
            kw = dict(h_appear=ha if na else None, flow_weights=flow_weights)
            a = dyn_ray_grads(p, fp, r, step, cot_of(S, seed), **kw)
            b = dyn_ray_grads(p, fp, r, step, cot_of(S, seed), rounding=round16, **kw)
            out[(S, T, na, Ld, Lf, ms)] = (rel_l2(b["o"][~ex_r], a["o"][~ex_r]), rel_l2(b["d"][~ex_r], a["d"][~ex_r]))
    return out


if __name__ == "__main__":      # the table behind test_pose_grad.FLOW_RAY_GRAD_TOL_FP16 (CPU only, about a minute)
    import test_pose_grad as tp
    res = flow_rounding_probe(tp.tdf.FLOW_PARITY, tp.DYN_STEP, (tp.tdf.W_CYCLE, tp.tdf.W_SPARSITY), tp.FLOW_RAYS, tp._cot)
    for k, (eo, ed) in res.items():
        print(k, f"rays_o {eo:.3e} rays_d {ed:.3e}")
    print("worst", max(max(v) for v in res.values()))
