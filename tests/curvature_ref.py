"""float64 restatement of the SDF curvature regulariser (``model.get_sdf_curvature_1d`` of
app/loss/sdf_curvature.py:69,75) in plain torch, taking the f32 inputs the kernels take -- the checker of tests/test_curvature.py --
and the small scene the reference's ``SDFCurvatureRegLoss`` is run on (shared with tests/golden/make_curvature_fixture.py).

The six steps:  n^ = n / max(|n|, 1e-12);  r^ likewise;  tau = n^ x r^ (not renormalised);  x' = clamp(x + eps tau, aabb), a constant;
(sdf', n') = forward_sdf_nablas(x');  curvature = acos(clamp(n^ . n'^, -c, c)) / pi  with c = 1 - 1e-6 AS ITS NEAREST f32
(1 - 1.0133e-6: the kernels compare in f32, and acos near 1 turns the 1.3 % of difference in 1 - c into 0.7 % of curvature)."""
import math

import numpy as np
import torch

NORM_MIN = 1e-12
DOT_MAX = float(np.float32(1.0 - 1e-6))
CURV_MIN = math.acos(DOT_MAX) / math.pi          # 4.5313716e-4: parallel normals
CURV_MAX = math.acos(-DOT_MAX) / math.pi         # 1 - 4.5313716e-4: antiparallel normals


def unit(v: torch.Tensor) -> torch.Tensor:
    """v / max(|v|, 1e-12); a vector shorter than 1e-12 is scaled by the CONSTANT 1e12 -- no gradient reaches it (the departure
    from ``F.normalize`` that DESIGN.md sec. 7 documents)."""
    v = v.double()
    ln = v.norm(dim=-1, keepdim=True)
    return torch.where(ln >= NORM_MIN, v / ln.clamp_min(NORM_MIN), (v / NORM_MIN).detach())


def shift(x, nablas, dirs, eps, aabb) -> torch.Tensor:
    """steps 1-4 -> x' [..., 3] float64 (no gradient)"""
    with torch.no_grad():
        tau = torch.linalg.cross(unit(nablas), unit(dirs), dim=-1)
        x2 = x.double() + float(np.float32(eps)) * tau
        lo, hi = aabb.double()[0], aabb.double()[1]
        return torch.minimum(torch.maximum(x2, lo), hi)


def dots(n0, n1) -> torch.Tensor:
    return (unit(n0) * unit(n1)).sum(-1)


def curvature(n0, n1) -> torch.Tensor:
    """step 6 -> [...] float64, differentiable w.r.t. n0 and n1"""
    return torch.acos(dots(n0, n1).clamp(-DOT_MAX, DOT_MAX)) / math.pi


def curvature_loss(n0, n1, clamp_max: float = 0.5) -> torch.Tensor:
    """``SDFCurvatureRegLoss.fn`` (app/loss/sdf_curvature.py:42): mean(min(curvature, clamp_max))"""
    return curvature(n0, n1).clamp_max(clamp_max).mean()


# ------------------------------------------------------------------------------------------------ the scene of test 6
SCENE_QP = dict(nablas_has_grad=True, num_coarse=8, num_fine=[4, 4], upsample_inv_s=64.0, upsample_inv_s_factors=[1, 4],
                upsample_use_estimate_alpha=True, march_cfg=dict(step_size=0.05, max_steps=128))
SCENE_EPS, SCENE_W, SCENE_ALPHA, SCENE_SEED = 0.05, 0.1, 1.0, 11


def scene_model(device, seed: int = 3):
    """A bumpy sphere (f32 field mode) with every voxel occupied, and 40 rays at it: -> (model, tested rays)"""
    from oracle import render as orr
    from util import look_at_cameras, make_params, model_from_params
    p = make_params(sdf_D=2, small=True, sphere=True, seed=seed, ln_inv_s=0.45, grid_bound=2e-2, noise_scale=1.0)
    m = model_from_params(p, device, precision="f32")
    m.accel.set_all_occupied()
    g = torch.Generator().manual_seed(seed)
    intr, c2w, WH = look_at_cameras(V=3, seed=seed)
    N = 40
    xy = torch.rand(N, 2, generator=g) * 0.5 + 0.25
    fidx = torch.randint(0, 3, (N,), generator=g)
    o, d = orr.pinhole_rays(xy, fidx, intr, c2w, WH)
    return m, o.to(device).contiguous(), d.to(device).contiguous()


def scene_query(m, o, d, with_net_x=True, **extra):
    tested = m.ray_test(o, d, near=0.01, far=None)
    qp = dict(SCENE_QP, **({} if with_net_x is None else dict(with_net_x=with_net_x)))
    cfg = dict(query_param=qp, with_rgb=False, with_normal=True, query_mode="march_occ_multi_upsample", perturb=False, **extra)
    return tested, m.ray_query(ray_tested=tested, config=cfg, return_details=True)
