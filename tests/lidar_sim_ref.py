"""Checkers of tests/test_lidar_sim.py: the formula of ``Lidar.get_all_rays`` (app/resources/observers/lidars.py:208-232) restated in
float64, the reference's own f32 torch composition of it (the yardstick of the accuracy bound), and the torch steps of
code_multi/tools/render.py:331-346 with the documented summation order of ``pts_local``."""
import torch


def angles(thetas, phis, mode):
    """per-ray (theta, phi) in the order of the reference: ``meshgrid(thetas, phis, indexing='xy')`` flattened, or the pairs"""
    if mode == "grid":
        Ts, Ps = torch.meshgrid(thetas, phis, indexing="xy")          # [n_az, n_beams]: beam fastest
        return Ts.reshape(-1), Ps.reshape(-1)
    return thetas.reshape(-1), phis.reshape(-1)


def _compose(T, P, c2w, axis):
    dx, dy, dz = c2w[:3, 0], c2w[:3, 1], c2w[:3, 2]
    if axis:          # lidars.py:221-224
        d = (torch.cos(T))[..., None] * dx + (torch.sin(T) * torch.sin(P))[..., None] * dy + \
            (torch.sin(T) * torch.cos(P) * -1)[..., None] * dz
    else:             # lidars.py:226-227
        d = (torch.sin(T) * torch.cos(P))[..., None] * dx + (torch.sin(T) * torch.sin(P))[..., None] * dy + \
            (torch.cos(T))[..., None] * dz
    return d


def rays_f64(thetas, phis, l2w, mode, axis):
    """-> rays_o [N,3] (f32, the translation bit for bit), rays_d [N,3] float64, theta_phi [N,2] f32"""
    T, P = angles(thetas.to(torch.float32), phis.to(torch.float32), mode)
    d = _compose(T.double(), P.double(), l2w.double(), axis)
    d = d / d.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    o = l2w[:3, 3].to(torch.float32).reshape(1, 3).expand(T.shape[0], 3)
    return o, d.reshape(-1, 3), torch.stack([T, P], dim=-1)


def rays_f32_torch(thetas, phis, l2w, mode, axis):
    """the reference's composition, op by op in f32 torch (lidars.py:218-230) -> rays_d [N,3] f32"""
    T, P = angles(thetas.to(torch.float32), phis.to(torch.float32), mode)
    d = _compose(T, P, l2w.to(torch.float32), axis)
    return torch.nn.functional.normalize(d, dim=-1).view(-1, 3)


def ray_errors(d, d64):
    """(largest component error, largest deviation of the norm from 1) of directions d against the float64 ones"""
    if d.shape[0] == 0:
        return 0.0, 0.0
    dd = d.double()
    return float((dd - d64).abs().max()), float((dd.norm(dim=-1) - 1.0).abs().max())


def returns(acc, depth, rays_o, rays_d, thr, w2l=None, rgb=None, ids=None):
    """render.py:331-346 in f32 torch: mask, masked gathers, ``o + d * r`` unfused; ``pts_local`` in the documented order
    ``((m0 x + m1 y) + m2 z) + t``, one torch operation per product and sum"""
    valid = acc > torch.tensor(thr, dtype=torch.float32)
    inds = torch.nonzero(valid)[:, 0]
    rg = depth[valid]
    out = dict(rays_inds=inds, ranges=rg, mask=acc[valid], pts_world=rays_o[valid] + rays_d[valid] * rg.unsqueeze(-1),
               range_image=torch.where(valid, depth, torch.zeros_like(depth)))
    if w2l is not None:
        x, y, z = out["pts_world"].unbind(-1)
        cols = []
        for k in range(3):
            a = w2l[k, 0] * x
            b = w2l[k, 1] * y
            c = w2l[k, 2] * z
            cols.append(((a + b) + c) + w2l[k, 3])
        out["pts_local"] = torch.stack(cols, dim=-1)
    if rgb is not None:
        out["rgb"] = rgb[valid]
    if ids is not None:
        out["ins_seg"] = ids[valid]
    return out


def bits_equal(a, b):
    """same shape, dtype and bits; NaNs the arithmetic PRODUCED may differ in sign and payload between processors and count as
    equal to each other (copies are compared with ``copies_equal``)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point():
        return bool(torch.equal(a, b))
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    ia, ib = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return bool(torch.equal(ia[~na], ib[~na]))


def copies_equal(a, b):
    """bit-equal, NaN payloads included"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.is_floating_point():
        return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))
    return bool(torch.equal(a, b))
