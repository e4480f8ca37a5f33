"""The SDF curvature regulariser (app/loss/sdf_curvature.py:42,69,75): the five ``nsim_curv_*`` kernels, the two
autograd functions of ``neuralsim_amd.losses``, ``get_sdf_curvature_1d`` on the models, ``with_net_x`` in the volume buffer, the
reference's own loss class on top of them, and the trainer's ``w_curvature`` -- against tests/curvature_ref.py (float64)."""
import math
import re
import types
from pathlib import Path

import numpy as np
import pytest
import torch

import curvature_ref as cref
import ref_glue
from neuralsim_amd import _lib, losses
from util import leaf, make_params, model_from_params

ROOT = Path(__file__).resolve().parent.parent
LOSS_BLOCK = int(re.search(r"#define LOSS_BLOCK (\d+)", (ROOT / "neuralsim_amd/csrc/loss_ops.hip").read_text()).group(1))
SIZES = [1, LOSS_BLOCK - 1, LOSS_BLOCK, LOSS_BLOCK + 1, 4 * LOSS_BLOCK + 3]
FIXTURE = ROOT / "tests" / "golden" / "curvature_fixture.pt"
needs_reference = ref_glue.needs_reference(ref_glue.reference_available(),
                                           reason="executes the reference's own loss class (emulator backend only); what it pins "
                                                  "is replayed from tests/golden/curvature_fixture.pt on both backends")


# ------------------------------------------------------------------------------------------------ 1. angle kernels
def _pairs(n, seed):
    """n pairs of vectors: random directions, norms log-uniform in [1e-3, 1e3], rejection-sampled to |n0^ . n1^| <= 0.999"""
    g = torch.Generator().manual_seed(seed)
    a, b = torch.empty(0, 3), torch.empty(0, 3)
    while a.shape[0] < n:
        def draw():
            v = torch.randn(2 * n + 8, 3, generator=g)
            return v / v.norm(dim=-1, keepdim=True) * 10.0 ** (torch.rand(2 * n + 8, 1, generator=g) * 6 - 3)
        ca, cb = draw(), draw()
        ok = cref.dots(ca, cb).abs() <= 0.999
        a, b = torch.cat([a, ca[ok]]), torch.cat([b, cb[ok]])
    return a[:n].contiguous(), b[:n].contiguous()


def _grad_err(got, ref):
    """max_i |got_i - ref_i| relative to the largest reference gradient norm"""
    scale = float(ref.norm(dim=-1).max())
    return float((got.detach().cpu().double() - ref).norm(dim=-1).max()) / scale


@pytest.fixture(scope="module")
def angle_refs():
    """float64 values and gradients per size, computed once: n -> (a, b, cot, curv, da, db, loss, dla, dlb)"""
    out = {}
    for n in SIZES:
        a, b = _pairs(n, seed=n)
        cot = torch.randn(n, generator=torch.Generator().manual_seed(n + 1)).double()
        ra, rb = leaf(a, dtype=torch.float64), leaf(b, dtype=torch.float64)
        curv = cref.curvature(ra, rb)
        da, db = torch.autograd.grad((curv * cot).sum(), [ra, rb])
        loss = cref.curvature_loss(ra, rb, 0.5)
        dla, dlb = torch.autograd.grad(loss * 1.7, [ra, rb])
        out[n] = tuple(t.detach() for t in (a, b, cot, curv, da, db, loss, dla, dlb))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_angle_kernels(backend, angle_refs, n):
    a, b, cot, curv, da, db = angle_refs[n][:6]
    x0, x1 = leaf(a, backend), leaf(b, backend)
    out = losses.sdf_curvature(x0, x1)
    assert out.shape == (n,) and out.dtype == torch.float32
    err = float((out.detach().cpu().double() - curv).abs().max())
    print(f"n={n} forward err {err:.3e}")
    assert err <= 2e-5
    (out * cot.float().to(backend)).sum().backward()
    e0, e1 = _grad_err(x0.grad, da), _grad_err(x1.grad, db)
    print(f"n={n} grad err {e0:.3e} {e1:.3e}")
    assert e0 <= 1e-4 and e1 <= 1e-4
    # dn0 = NULL: only the second input asks for a gradient
    y0, y1 = a.to(backend), leaf(b, backend)
    (losses.sdf_curvature(y0, y1) * cot.float().to(backend)).sum().backward()
    assert y0.grad is None and _grad_err(y1.grad, db) <= 1e-4
    # the entry point itself with dn1 = NULL
    d0 = torch.empty(n, 3, device=backend)
    _lib.call("nsim_curv_angle_bwd", _lib.ptr(y0), _lib.ptr(y1.detach()), _lib.ptr(cot.float().to(backend)), n, _lib.ptr(d0), None)
    assert _grad_err(d0, da) <= 1e-4
    # [.., 3] shapes keep their shape
    if n == LOSS_BLOCK:
        z0 = leaf(a.view(16, n // 16, 3), backend)
        o2 = losses.sdf_curvature(z0, b.to(backend).view(z0.shape))
        assert o2.shape == z0.shape[:-1]
        o2.sum().backward()
        assert z0.grad.shape == z0.shape


@pytest.mark.parametrize("n", SIZES)
def test_fused_loss_kernels(backend, angle_refs, n):
    a, b = angle_refs[n][:2]
    loss, dla, dlb = angle_refs[n][6:]
    x0, x1 = leaf(a, backend), leaf(b, backend)
    out = losses.sdf_curvature_loss(x0, x1, 0.5)
    rel = abs(float(out.detach()) - float(loss)) / abs(float(loss))
    print(f"n={n} fused forward rel err {rel:.3e}")
    assert out.shape == () and rel <= 1e-5
    (out * 1.7).backward()
    e0, e1 = _grad_err(x0.grad, dla), _grad_err(x1.grad, dlb)
    print(f"n={n} fused grad err {e0:.3e} {e1:.3e}")
    assert e0 <= 1e-4 and e1 <= 1e-4
    y0, y1 = a.to(backend), leaf(b, backend)                    # dn0 = NULL
    (losses.sdf_curvature_loss(y0, y1) * 1.7).backward()
    assert y0.grad is None and _grad_err(y1.grad, dlb) <= 1e-4


def test_losses_refuse_host_tensors():
    a = torch.randn(5, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        losses.sdf_curvature(a, a)
    with pytest.raises(RuntimeError, match="no CPU path"):
        losses.sdf_curvature_loss(a, a)


# ------------------------------------------------------------------------------------------------ 2. edge cases
def test_edge_cases_exact(backend):
    v = torch.tensor([[0.3, -1.2, 0.7], [4e2, 1e2, -3e2], [0.0, 0.0, 0.0], [1e-3, 2e-3, -1e-3]])
    n0 = torch.stack([v[0], v[1], v[2], v[3]])
    n1 = torch.stack([2.5 * v[0], -0.3 * v[1], v[0], v[2]])         # parallel, antiparallel, zero n0, zero n1
    want = torch.tensor([np.float32(cref.CURV_MIN), np.float32(cref.CURV_MAX), 0.5, 0.5], dtype=torch.float32)
    x0, x1 = leaf(n0, backend), leaf(n1, backend)
    c = losses.sdf_curvature(x0, x1)
    assert bool(torch.isfinite(c).all())
    assert torch.equal(c.detach().cpu(), want), (c.detach().cpu() - want)
    c.sum().backward()
    y0, y1 = leaf(n0, backend), leaf(n1, backend)
    fused = losses.sdf_curvature_loss(y0, y1, 0.75)
    assert abs(float(fused) - float(want.double().clamp_max(0.75).mean())) <= 1e-6
    fused.backward()
    for g in (x0.grad, x1.grad, y0.grad, y1.grad):                  # all four gradients: exactly zero (and not NaN)
        assert torch.equal(g.cpu(), torch.zeros(4, 3))


def test_result_may_be_clamped_in_place(backend):
    a, b = _pairs(300, seed=5)
    x0, x1 = leaf(a, backend), leaf(b, backend)
    c = losses.sdf_curvature(x0, x1)
    assert c._base is None                                          # not a view
    full = c.detach().clone()
    c.clamp_max_(0.5).abs().mean().backward()                       # SDFCurvatureRegLoss.fn, app/loss/sdf_curvature.py:42
    ra, rb = leaf(a, dtype=torch.float64), leaf(b, dtype=torch.float64)
    cref.curvature_loss(ra, rb).backward()
    assert 0 < int((full > 0.5).sum()) < 300
    assert _grad_err(x0.grad, ra.grad) <= 1e-4 and _grad_err(x1.grad, rb.grad) <= 1e-4


# ------------------------------------------------------------------------------------------------ 3. shift kernel
AABB_BOX = torch.tensor([[-1.0, -0.5, -2.0], [1.5, 0.5, 1.0]])


def _box_model(backend):
    from neuralsim_amd.fields.neus import OccGridAccel
    m = model_from_params(make_params(sdf_D=1, small=True, sphere=True, seed=1), backend, precision="f32")
    m.accel = OccGridAccel(AABB_BOX, resolution=[8, 8, 8], device=backend)
    return m


def test_shift_kernel(backend):
    m = _box_model(backend)
    eps, n = 0.05, 4 * LOSS_BLOCK + 3
    g = torch.Generator().manual_seed(8)
    lo, hi = AABB_BOX[0], AABB_BOX[1]
    x = lo + torch.rand(n, 3, generator=g) * (hi - lo)
    face = torch.arange(n) % 8                                      # 6 of every 8 points sit within eps of a face of the box
    for f in range(6):
        k, side = f // 2, f % 2
        rows = face == f
        off = torch.rand(int(rows.sum()), generator=g) * eps
        x[rows, k] = (hi[k] - off) if side else (lo[k] + off)
    nab = torch.randn(n, 3, generator=g) * 10.0 ** (torch.rand(n, 1, generator=g) * 4 - 2)
    dirs = torch.randn(n, 3, generator=g)
    ref = cref.shift(x, nab, dirs, eps, AABB_BOX)
    free = x.double() + eps * torch.linalg.cross(cref.unit(nab), cref.unit(dirs), dim=-1)
    assert int(((free < lo) | (free > hi)).any(-1).sum()) > n // 8  # the clamp is exercised
    dv = lambda t: t.to(backend)                                    # noqa: E731
    got = m._curvature_neighbours(dv(x), dv(nab), eps, dirs=dv(dirs))
    err = float((got.cpu().double() - ref).abs().max())
    print(f"shift err {err:.3e}")
    assert got.shape == (n, 3) and err <= 1e-6
    assert bool(((got.cpu() >= lo) & (got.cpu() <= hi)).all())
    assert torch.equal(got, m._curvature_neighbours(dv(x), dv(nab), eps, dirs=dv(dirs)))
    mk = lambda: torch.Generator(device=backend).manual_seed(77)    # noqa: E731
    r1 = m._curvature_neighbours(dv(x), dv(nab), eps, generator=mk())
    r2 = m._curvature_neighbours(dv(x), dv(nab), eps, generator=mk())
    assert torch.equal(r1, r2) and not torch.equal(r1, got)


# ------------------------------------------------------------------------------------------------ 4. models
def _rough_lotd(backend):
    # a randomly initialised table, U(-0.05, 0.05), under the random (not the sphere) decoder
    p = make_params(sdf_D=2, small=True, sphere=False, seed=21, grid_bound=5e-2, noise_scale=1.0)
    return model_from_params(p, backend, precision="f32")


def _rough_permuto(backend):
    from neuralsim_amd.fields.permuto_neus import PermutoNeuSModel
    cfg = dict(type="multi_res", n_levels=6, n_feats=2, log2_hashmap_size=11, coarsest_res=2.0, finest_res=24.0,
               apply_random_shifts_per_level=True, seed=5)
    return PermutoNeuSModel(permuto_auto_compute_cfg=cfg, sdf_D=1, precision="f32", param_bound=1.0, seed=9).to(backend)


@pytest.mark.parametrize("kind", ["lotd", "permuto"])
def test_model_get_sdf_curvature_1d(backend, kind):
    """``get_sdf_curvature_1d(x, nablas, eps, dirs=)`` against the restatement composed from the model's own ``forward_sdf_nablas``
    (both sides run the same field kernels; only the pointwise part differs), 1000 uniform points, eps = 0.05, on a randomly
    initialised table.  Share of points with |n^ . n'^| < 0.999 under the restatement (emulator): lotd 100.0 %, permuto 95.1 %
    (the test requires 90 %: on a smooth field every dot product sits inside the clamp and nothing is compared)."""
    m = _rough_lotd(backend) if kind == "lotd" else _rough_permuto(backend)
    eps, n = 0.05, 1000
    g = torch.Generator().manual_seed(4)
    aabb = m.accel.aabb.cpu()
    x = (aabb[0] + torch.rand(n, 3, generator=g) * (aabb[1] - aabb[0])).to(backend)
    dirs = torch.randn(n, 3, generator=g).to(backend)
    cot = torch.randn(n, generator=g)
    table, params = m.encoding.flattened_params, [m.encoding.flattened_params, m.sdf_w, m.sdf_b]

    def grads(curv):
        gs = torch.autograd.grad((curv * cot.to(curv)).sum(), params)
        return [t.detach().cpu().double() for t in gs]
    # restatement
    nab = m.forward_sdf_nablas(x)["nablas"]
    x2 = cref.shift(x.cpu(), nab.detach().cpu(), dirs.cpu(), eps, aabb).float().to(backend)
    nab2 = m.forward_sdf_nablas(x2)["nablas"]
    d = cref.dots(nab.detach().cpu(), nab2.detach().cpu())
    share = float((d.abs() < 0.999).double().mean())
    print(f"{kind}: share of points with |dot| < 0.999: {share:.3f}")
    assert share >= 0.9
    ref = cref.curvature(nab.cpu(), nab2.cpu())
    g_ref = grads(ref)
    # product
    nab_p = m.forward_sdf_nablas(x)["nablas"]
    got = m.get_sdf_curvature_1d(x, nab_p, eps, dirs=dirs)
    assert got.shape == (n,) and got.dtype == torch.float32
    free = d.abs() < cref.DOT_MAX
    err = float((got.detach().cpu().double() - ref.detach())[free].abs().max())
    print(f"{kind}: forward err {err:.3e} on {int(free.sum())} unclamped points")
    assert err <= 2e-5
    for name, a, b in zip(("table", "sdf_w", "sdf_b"), grads(got), g_ref):
        rel = float((a - b).abs().max() / b.abs().max())
        print(f"{kind}: d {name} rel max-norm err {rel:.3e}")
        assert float(b.abs().max()) > 0 and rel <= 1e-3
    assert table.grad is None


def test_batched_models_refuse_by_name():
    from neuralsim_amd.fields.batched_neus import BatchedLoTDNeuSModel
    from neuralsim_amd.fields.batched_permuto_neus import BatchedPermutoNeuSModel
    from nr3d_lib.models.fields.neus import LoTDNeuSModel, PermutoNeuSModel          # the names the reference constructs
    assert callable(LoTDNeuSModel.get_sdf_curvature_1d) and callable(PermutoNeuSModel.get_sdf_curvature_1d)
    z = torch.zeros(2, 3)
    for cls in (BatchedLoTDNeuSModel, BatchedPermutoNeuSModel):
        with pytest.raises(NotImplementedError, match=cls.__name__):
            cls.get_sdf_curvature_1d(object.__new__(cls), z, z, eps=1e-4)


# ------------------------------------------------------------------------------------------------ 5. with_net_x
def test_with_net_x(backend):
    m, o, d = cref.scene_model(backend)
    with torch.no_grad():
        _, r_none = cref.scene_query(m, o, d, with_net_x=None)
        _, r_off = cref.scene_query(m, o, d, with_net_x=False)
        tested, r_on = cref.scene_query(m, o, d, with_net_x=True)
    vb0, vb_off, vb1 = r_none["volume_buffer"], r_off["volume_buffer"], r_on["volume_buffer"]
    assert set(vb0) == {"type", "rays_inds_hit", "pack_infos_hit", "t", "opacity_alpha", "nablas", "sdf"}     # today's keys
    assert set(vb_off) == set(vb0) and set(vb1) == set(vb0) | {"net_x"}
    for k in vb0:
        for other in (vb_off, vb1):
            assert vb0[k] == other[k] if isinstance(vb0[k], str) else torch.equal(vb0[k], other[k]), k
    S = vb1["t"].shape[0]
    ridx = r_on["details"]["ridx"]
    want = tested["rays_o"][ridx].double() + vb1["t"].double()[:, None] * tested["rays_d"][ridx].double()
    assert S > 100 and vb1["net_x"].shape == (S, 3) and vb1["net_x"].requires_grad is False
    assert float((vb1["net_x"].double() - want).abs().max()) <= 1e-6
    # with gradients enabled the positions are still a constant of the step
    _, r_g = cref.scene_query(m, o, d, with_net_x=True)
    assert r_g["volume_buffer"]["nablas"].requires_grad and not r_g["volume_buffer"]["net_x"].requires_grad


# ------------------------------------------------------------------------------------------------ 6. the reference's class
def _class_inputs(m, o, d):
    _, ret = cref.scene_query(m, o, d, with_net_x=True)
    return dict(raw_per_obj_model=dict(main=dict(volume_buffer=ret["volume_buffer"], class_name="Main", model_id="main")))


@needs_reference
def test_reference_sdf_curvature_reg_loss_unchanged(backend):
    """``SDFCurvatureRegLoss`` (app/loss/sdf_curvature.py:24-78, loaded unchanged) with ``on_uniform_samples=False`` and
    ``alpha_loss_on_render`` 1 -- the one branch that can run: its uniform branch indexes ``uniform_samples['net_x']`` on a dict
    keyed by class name -- on a ``ray_query`` with ``with_net_x``: w * mean(min(restatement, 0.5)), and a table gradient."""
    m, o, d = cref.scene_model(backend)
    ret = _class_inputs(m, o, d)
    vb = ret["raw_per_obj_model"]["main"]["volume_buffer"]
    scene = types.SimpleNamespace(asset_bank=dict(main=m))
    with ref_glue.reference_loss_module("sdf_curvature") as mod:
        loss_mod = mod.SDFCurvatureRegLoss({"Main": {"w": cref.SCENE_W, "alpha_loss_on_render": cref.SCENE_ALPHA}}, ["Main"],
                                           on_uniform_samples=False, eps=cref.SCENE_EPS)
        torch.manual_seed(cref.SCENE_SEED)
        out = loss_mod(scene, ret, {}, {}, {}, 0)
    assert set(out) == {"loss_sdf_curvature_reg.Main.render"}
    got = out["loss_sdf_curvature_reg.Main.render"]
    torch.manual_seed(cref.SCENE_SEED)
    S = vb["t"].shape[0]
    dirs = torch.randn(S, 3)
    x2 = cref.shift(vb["net_x"].cpu(), vb["nablas"].detach().cpu(), dirs, cref.SCENE_EPS, m.accel.aabb.cpu()).float().to(backend)
    with torch.no_grad():
        nab2 = m.forward_sdf_nablas(x2)["nablas"]
    want = cref.SCENE_W * cref.SCENE_ALPHA * float(cref.curvature_loss(vb["nablas"].detach().cpu(), nab2.cpu()))
    print(f"class {float(got):.8e} restatement {want:.8e}")
    assert abs(float(got) - want) <= 1e-5 * abs(want)
    got.backward()
    gt_ = m.encoding.flattened_params.grad
    assert gt_ is not None and bool(torch.isfinite(gt_).all()) and float(gt_.abs().max()) > 0


def test_reference_class_scalar_replayed_from_the_fixture(backend):
    """The frozen run of the test above (tests/golden/make_curvature_fixture.py: the model's weights, rays, the drawn
    directions, the class's scalar) through this package's own loss: ``ray_query`` with ``with_net_x`` ->
    ``get_sdf_curvature_1d`` -> ``clamp_max_(0.5).mean()``.  Bound 1e-4 relative: both runs are the f32 field mode of the same
    kernels, so they differ by the rounding of the device's transcendentals and fused arithmetic, ~1e-6 relative in the nablas,
    amplified by at most 22.4 / pi through the acos of the unclamped pairs."""
    fx = torch.load(FIXTURE)
    m, o, d = cref.scene_model(backend)
    with torch.no_grad():
        m.encoding.flattened_params.copy_(fx["table"].float().to(backend))
        for k in ("sdf_w", "sdf_b"):
            getattr(m, k).copy_(fx[k].to(backend))
    m._invalidate_packs()
    assert torch.equal(o.cpu(), fx["rays_o"]) and torch.equal(d.cpu(), fx["rays_d"])
    _, ret = cref.scene_query(m, o, d, with_net_x=True)
    vb = ret["volume_buffer"]
    assert vb["t"].shape[0] == fx["dirs"].shape[0]
    c = m.get_sdf_curvature_1d(vb["net_x"], vb["nablas"], eps=float(fx["eps"]), dirs=fx["dirs"].to(backend))
    got = float(fx["w"]) * c.clamp_max_(0.5).abs().mean()
    print(f"replay {float(got):.8e} class {float(fx['loss']):.8e}")
    assert abs(float(got) - float(fx["loss"])) <= 1e-4 * abs(float(fx["loss"]))
    fused = float(fx["w"]) * losses.sdf_curvature_loss(vb["nablas"], m.forward_sdf_nablas(
        m._curvature_neighbours(vb["net_x"], vb["nablas"], float(fx["eps"]), dirs=fx["dirs"].to(backend)))["nablas"])
    assert abs(float(fused) - float(got)) <= 1e-5 * abs(float(got))
    got.backward()
    assert float(m.encoding.flattened_params.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 7. trainer
def _tiny_trainer(backend, **kw):
    from neuralsim_amd.fields.neus import LoTDNeuSModel
    from neuralsim_amd.graphics.cameras import look_at_cameras
    from neuralsim_amd.trainer import RenderTrainer
    from util import SMALL_RES
    torch.manual_seed(0)                                            # (the initialisation noise and the occupancy warm-up draw from it)
    qp = dict(nablas_has_grad=True, num_coarse=8, num_fine=[4, 4], upsample_inv_s=64.0, upsample_inv_s_factors=[1, 4],
              upsample_use_estimate_alpha=True, march_cfg=dict(step_size=0.05, max_steps=128))
    m = LoTDNeuSModel(lod_res=SMALL_RES, log2_hashmap_size=10, sdf_D=2, precision="fp16", ln_inv_s_init=0.3,
                      accel_cfg=dict(resolution=(16, 16, 16), update_from_net_cfg=dict(num_steps=1, num_pts=2048),
                                     update_from_samples_cfg={}, n_steps_between_update=10 ** 9, n_steps_warmup=10 ** 9),
                      ray_query_cfg=dict(query_mode="march_occ_multi_upsample", query_param=qp), seed=42).to(backend)
    m.geometric_init_sphere(0.5, noise_scale=1.0)
    m.accel.init(m.query_sdf, num_steps=1, num_pts=4096)
    intr, c2w, WH = look_at_cameras(V=4, seed=1, device=backend)
    tr = RenderTrainer(m, intr, c2w, WH, num_rays=24, lr=2e-3, num_uniform=64, perturb=True, target_sphere_radius=0.5,
                       curvature_eps=0.05, **kw)
    return m, tr


def test_trainer_curvature_term(backend):
    m, tr = _tiny_trainer(backend, w_curvature=0.05)
    assert not tr._fused_ok()                                       # the term runs on the autograd path
    loss = tr.train_step(0)
    assert math.isfinite(float(loss))
    parts = tr.loss_parts
    assert "loss_curvature" in parts and 0.0 < float(parts["loss_curvature"]) <= 0.5
    want = float(parts["loss_rgb"]) + tr.w_eikonal * float(parts["loss_eikonal"]) + 0.05 * float(parts["loss_curvature"])
    assert abs(float(loss) - want) <= 1e-5 * abs(want)
    g = m.encoding.flattened_params.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    # the same step without the term leaves another table gradient: the term reached the table
    m0, tr0 = _tiny_trainer(backend, w_curvature=0.0, fused_step=False)
    loss0 = tr0.train_step(0)
    assert "loss_curvature" not in tr0.loss_parts and abs(float(loss0) - (want - 0.05 * float(parts["loss_curvature"]))) <= 1e-4
    assert float((g - m0.encoding.flattened_params.grad).abs().max()) > 0


def test_trainer_curvature_converges_on_a_fixed_objective(backend):
    """One batch, rewound jitter streams (util.steps_on_a_fixed_objective): the same pixels, uniform points and tangent directions
    every step, so the curvature term is one fixed function of the parameters -- lower after 20 Adam steps than at step 0."""
    from util import steps_on_a_fixed_objective
    m, tr = _tiny_trainer(backend, w_curvature=0.05)
    xy, fidx, gt = tr.sample_batch()
    tr.sample_batch = lambda: (xy, fidx, gt)
    curv = []
    step = tr.train_step

    def recording_step(it):
        out = step(it)
        curv.append(float(tr.loss_parts["loss_curvature"]))
        return out
    tr.train_step = recording_step
    losses_ = steps_on_a_fixed_objective(tr, range(21))
    assert all(l == l for l in losses_) and len(curv) == 21
    print("curvature term", ["%.5f" % c for c in curv])
    assert curv[-1] < curv[0], curv


def test_trainer_without_the_term_is_unchanged(backend):
    m, tr = _tiny_trainer(backend)                                  # w_curvature defaults to 0
    assert tr.w_curvature == 0.0 and tr._fused_ok() == tr.fused_step
    losses_ = [float(tr.train_step(it)) for it in range(2)]
    assert all(math.isfinite(l) for l in losses_) and "loss_curvature" not in tr.loss_parts
