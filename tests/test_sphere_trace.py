"""``query_mode: sphere_trace``: the persistent tracer kernel (csrc/field.hip ``k_sphere_trace``) through
``LoTDNeuSModel.ray_query`` / ``model.tracer`` against the restatement of tests/sphere_trace_ref.py, the host-loop replay, the
existing no-grad query and the volume renderer.  Scene: the geometric-init "bumpy sphere" of tests/util.py, object preset."""
import pytest
import torch

import ref_glue
import sphere_trace_ref as sref
from oracle import render as orr
from util import look_at_cameras, make_params, model_from_params

AABB = torch.tensor([[-1.0, -1, -1], [1.0, 1, 1]])
RES = [32, 32, 32]
MARCH = dict(step_size=0.02, max_steps=512)
# the object preset (app/visualizer/gui_runner_single_cuboid.py:91-104)
PRESET = dict(distance_scale=1.0, min_step=0.002, hit_threshold=1e-4, max_march_iters=500, drop_alive_rate=0.0,
              tail_sample_threshold=20000, tail_sample_step_size=None, debug=True)
QP_VOLUME = dict(nablas_has_grad=False, num_coarse=16, num_fine=[4, 4, 8], upsample_inv_s=64.0, upsample_inv_s_factors=[1, 4, 16],
                 upsample_use_estimate_alpha=True, march_cfg=MARCH)
# fused vs level-major no-grad query, tests/test_field.py (``atol=2e-6``): two evaluations of the same SDF by the same decoder
TOL_SAME_DECODER = 2e-6
# oracle vs kernel SDF, tests/test_field.py: f32 field 2e-5 (1 + max|sdf|); split-precision sampling query 4e-6 (1 + max|sdf|)
EPS_ORACLE = dict(f32=2e-5, fp16=4e-6)
needs_reference = ref_glue.needs_reference(ref_glue.reference_available(), reason="executes the reference's own renderer source (emulator backend only)")


def _scene(backend, precision="f32", N=400, seed=3, spread=0.5):
    p = make_params(sdf_D=2, small=True, sphere=True, seed=seed, ln_inv_s=0.45, grid_bound=2e-2, noise_scale=1.0)
    g = torch.Generator().manual_seed(seed)
    intr, c2w, WH = look_at_cameras(V=3, seed=seed)
    xy = torch.rand(N, 2, generator=g) * spread + (0.5 - spread / 2)
    o, d = orr.pinhole_rays(xy, torch.randint(0, 3, (N,), generator=g), intr, c2w, WH)
    from neuralsim_amd.fields.neus import OccGridAccel
    model = model_from_params(p, backend, precision=precision)
    model.accel = OccGridAccel(AABB, resolution=RES, device=backend)
    val, occ = orr.build_occ_grid(p, AABB[0], AABB[1], RES, n_pts=2 ** 17, n_steps=2, inv_s=64.0)
    # (4 points per voxel and |sdf| < 0.04 > half a voxel: a closed shell -- with holes in it a ray's first occupied point lies on the far side)
    model.accel.occ_val.copy_(val.to(backend))
    model.accel.pack_bits()
    model.ray_query_cfg = dict(query_mode="march_occ_multi_upsample", query_param=QP_VOLUME)
    h = torch.randn(N, 4, generator=g) * 0.3
    return p, model, o.to(backend).contiguous(), d.to(backend).contiguous(), h.to(backend), occ


def _cfg(**over):
    qp = dict(PRESET)
    qp.update(over)
    return dict(query_mode="sphere_trace", query_param=qp, with_rgb=True, with_normal=True, _render=True)


def _trace(model, o, d, **over):
    tested = model.ray_test(o, d, near=0.01, far=None)
    ret = model.ray_query(ray_tested=tested, config=_cfg(**over), return_details=True)
    return tested, ret


@pytest.mark.parametrize("precision", ["f32", "fp16"])
def test_buffer_has_one_opaque_sample_per_hit_ray(backend, precision):
    _, model, o, d, h, _ = _scene(backend, precision)
    o[::7] += torch.tensor([0.0, 4.0, 0.0], device=backend)          # some rays miss the box
    tested = model.ray_test(o, d, near=0.01, far=None, rays_h_appear=h)
    ret = model.ray_query(ray_tested=tested, config=_cfg(), return_details=True)
    vb, det = ret["volume_buffer"], ret["details"]
    assert vb["type"] == "packed" and det["status"].shape == (tested["num_rays"],) and det["status"].dtype == torch.uint8
    hit = (det["status"] == 1).nonzero()[:, 0]
    H = hit.shape[0]
    assert 50 < H < tested["num_rays"]
    assert torch.equal(vb["rays_inds_hit"], tested["rays_inds"][hit]) and bool((vb["rays_inds_hit"][1:] > vb["rays_inds_hit"][:-1]).all())
    assert torch.equal(vb["pack_infos_hit"][:, 1].cpu(), torch.ones(H, dtype=torch.long))
    assert torch.equal(vb["pack_infos_hit"][:, 0].cpu(), torch.arange(H))
    assert vb["t"].shape == (H,) and torch.equal(vb["t"], det["t"][hit])
    assert torch.equal(vb["opacity_alpha"].cpu(), torch.ones(H))
    assert vb["sdf"].shape == (H,) and vb["nablas"].shape == (H, 3) and vb["rgb"].shape == (H, 3)
    assert not (vb["sdf"].requires_grad or vb["rgb"].requires_grad)
    for k in ("sdf", "nablas", "rgb"):
        assert bool(torch.isfinite(vb[k]).all()), k
    # the with-grad-capable query at the hit points is below the threshold as well: it and the tracer's query are each within
    # test_field.py's tolerance of the oracle (f32 2e-5, fp16 4e-3, times 1 + max|sdf| <= 2)
    assert float(vb["sdf"].max()) <= PRESET["hit_threshold"] + 2 * 2 * dict(f32=2e-5, fp16=4e-3)[precision]
    r = ret["rendered"]
    assert torch.equal(r["mask_volume"].cpu(), torch.ones(H)) and torch.allclose(r["depth_volume"], vb["t"])
    # rays that all miss the box
    far_o = o + torch.tensor([0.0, 6.0, 0.0], device=backend)
    tested0 = model.ray_test(far_o, d, near=0.01, far=None)
    assert tested0["num_rays"] == 0
    ret0 = model.ray_query(ray_tested=tested0, config=_cfg(), return_details=True)
    assert ret0["volume_buffer"]["type"] == "empty"


@pytest.mark.parametrize("precision", ["f32", "fp16"])
def test_hits_lie_on_the_surface_of_the_existing_query(backend, precision):
    """Self-consistency with the existing no-grad query (the one the tracer steps on: ``tracer.query_sdf``, the model's
    sampling-precision query; with an f32 field that is ``model.query_sdf`` itself).  tol: TOL_SAME_DECODER."""
    _, model, o, d, _, _ = _scene(backend, precision)
    tested, ret = _trace(model, o, d)
    det = ret["details"]
    x = tested["rays_o"] + det["t"][:, None] * tested["rays_d"]
    q = model.tracer.query_sdf(x)
    hit, queried = det["status"] == 1, det["n_steps"] > 0
    print(f"[{precision}] max |sdf_out - query_sdf| = {float((q - det['sdf_nograd'])[queried].abs().max()):.3e}; "
          f"max query_sdf on hits = {float(q[hit].max()):.3e}")
    assert bool((q[hit] <= PRESET["hit_threshold"] + TOL_SAME_DECODER).all())
    assert bool(((q - det["sdf_nograd"])[queried].abs() <= TOL_SAME_DECODER).all())
    assert bool(torch.isnan(det["sdf_nograd"][~queried]).all()) and torch.equal(det["t"][~queried], tested["near"][~queried])
    if precision == "f32":
        qm = model.query_sdf(x)
        assert bool((qm[hit] <= PRESET["hit_threshold"] + TOL_SAME_DECODER).all())
        assert bool(((qm - det["sdf_nograd"])[queried].abs() <= TOL_SAME_DECODER).all())


@pytest.mark.parametrize("precision", ["f32", "fp16"])
def test_parity_with_the_restatement(backend, precision):
    """The restatement runs three times, its SDF shifted by 0 and +-eps (the oracle-vs-kernel SDF tolerance of test_field.py
    for the precision of the tracer's query); on the rays whose status and n_steps agree in all three -- at least 95 % -- the
    kernel's status and n_steps equal the restatement's and t lies within the spread of the three runs plus the f32 rounding
    of n_steps additions.  (Restatement alone on this scene and seed: 1.0 % unstable with the f32 eps, 0.25 % with the split one.)"""
    p, model, o, d, _, occ = _scene(backend, precision)
    tested, ret = _trace(model, o, d)
    det = {k: v.cpu() for k, v in ret["details"].items()}
    oo, dd, near, far = (tested[k].cpu() for k in ("rays_o", "rays_d", "near", "far"))
    kw = dict(step=MARCH["step_size"], max_steps=MARCH["max_steps"], distance_scale=PRESET["distance_scale"],
              min_step=PRESET["min_step"], hit_threshold=PRESET["hit_threshold"], max_march_iters=PRESET["max_march_iters"])
    eps = EPS_ORACLE[precision] * (1.0 + 1.0)          # |sdf| <= 1 inside the box of the unit-scale sphere scene (checked below)
    runs = [sref.trace(p, oo, dd, near, far, occ, AABB[0], AABB[1], RES, sdf_shift=s, **kw) for s in (0.0, eps, -eps)]
    assert float(torch.nan_to_num(runs[0]["sdf"]).abs().max()) <= 1.0
    stable, spread = sref.stable_rays(runs)
    unstable = 1.0 - float(stable.float().mean())
    r0 = runs[0]
    dt = (r0["t"] - det["t"]).abs()
    tol_t = spread + det["n_steps"].float() * 2.0 ** -23 * det["t"].abs().clamp_min(1.0)
    print(f"[{precision}] unstable {unstable:.4f}; status equal on {float((r0['status'] == det['status']).float().mean()):.4f} of all rays; "
          f"max |t - t_ref| on stable rays {float(dt[stable].max()):.3e} (max spread {float(spread[stable].max()):.3e})")
    assert unstable <= 0.05
    assert int((r0["status"] == 1).sum()) > 100 and int((r0["status"] == 2).sum()) > 100
    assert torch.equal(det["status"][stable], r0["status"][stable])
    assert torch.equal(det["n_steps"][stable], r0["n_steps"][stable])
    assert bool((dt <= tol_t)[stable].all())


def test_results_do_not_depend_on_the_schedule(backend):
    """Two calls are bit-identical; permuting the rays permutes the outputs bit-identically (other tile-mates, other waves)."""
    _, model, o, d, _, _ = _scene(backend, "fp16")
    tested, ret = _trace(model, o, d)
    _, ret2 = _trace(model, o, d)
    det, det2 = ret["details"], ret2["details"]
    perm = torch.randperm(o.shape[0], generator=torch.Generator().manual_seed(1)).to(backend)
    tested_p, ret_p = _trace(model, o[perm].contiguous(), d[perm].contiguous())
    assert tested_p["num_rays"] == tested["num_rays"]
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(perm.shape[0], device=backend)
    # tested ray i of the first call is tested ray rank[i] of the permuted call
    pos = torch.empty(o.shape[0], dtype=torch.long, device=backend)
    pos[tested_p["rays_inds"]] = torch.arange(tested_p["num_rays"], device=backend)
    rank = pos[inv[tested["rays_inds"]]]
    for k in ("status", "n_steps", "t", "sdf_nograd"):
        a, b, c = det[k], det2[k], ret_p["details"][k][rank]
        if a.is_floating_point():
            a, b, c = (v.view(torch.int32) for v in (a, b, c))
        assert torch.equal(a, b), k
        assert torch.equal(a, c), k


@pytest.mark.parametrize("precision", ["f32", "fp16"])
def test_host_replay_agrees_with_the_kernel(backend, precision):
    """``tracer.trace(..., debug_replay=True)``: the host loop over the no-grad query.  Same decoder, same steps: status and
    n_steps are equal and t agrees within TOL_SAME_DECODER per step.  Observed on the emulator and on the MI355X: bit-equal."""
    _, model, o, d, _, _ = _scene(backend, precision)
    tested = model.ray_test(o, d, near=0.01, far=None)
    tr = model.tracer
    hits = tr.trace(tested, None, query_param=dict(PRESET, march_cfg=MARCH))
    dbg = {}
    hits_r = tr.trace(tested, tr.query_sdf, debug_output=dbg, debug_replay=True, query_param=dict(PRESET, march_cfg=MARCH))
    a, b = hits["details"], hits_r["details"]
    print(f"[{precision}] max |t_kernel - t_replay| = {float((a['t'] - b['t']).abs().max()):.3e}")
    assert torch.equal(a["status"], b["status"]) and torch.equal(a["n_steps"], b["n_steps"])
    assert bool(((a["t"] - b["t"]).abs() <= TOL_SAME_DECODER * PRESET["distance_scale"] * a["n_steps"].float().clamp_min(1)).all())
    assert torch.equal(hits["rays_inds_hit"], hits_r["rays_inds_hit"]) and hits["num_rays_hit"] == int((a["status"] == 1).sum())
    # the recorded iterations: ray 0's occupied runs and, per iteration, the state of the rays queried in it
    assert dbg["segs"].dim() == 2 and dbg["segs"].shape[1] == 2 and bool((dbg["segs"][:, 1] > dbg["segs"][:, 0]).all())
    assert len(dbg["trace_data"]) == int(a["n_steps"].max())
    last = dbg["trace_data"][-1]
    assert set(last["rays_alive"]) >= {"t", "n_steps", "status"} and last["d"].shape == last["rays_alive"]["t"].shape
    # a callable that returns a dict, as ``obj_model.forward_sdf`` does (inspect_rendering.py:262)
    hits_d = tr.trace(tested, lambda x: dict(sdf=tr.query_sdf(x)), debug_output={}, debug_replay=True,
                      query_param=dict(PRESET, march_cfg=MARCH))
    assert torch.equal(hits_d["details"]["status"], b["status"])


def test_depth_agrees_with_volume_rendering(backend):
    """Volume rendering at ``forward_inv_s = 64000`` (eval_lidar's first-surface approximation) and the tracer on the same rays:
    where both masks exceed 0.5 the depths differ by at most 0.54 march steps.  Measured on the emulator against the existing
    renderer: max 0.27 step (270 rays; median 0.08) -> x2 margin for the fp16 device path = 0.54."""
    _, model, o, d, _, _ = _scene(backend, "fp16")
    tested, ret = _trace(model, o, d)
    vol = model.ray_query(ray_tested=tested, config=dict(query_mode="march_occ_multi_upsample", query_param=QP_VOLUME,
                                                         with_rgb=False, _render=True, forward_inv_s=64000.0,
                                                         depth_use_normalized_vw=True))
    R = tested["num_rays"]
    hit = (ret["details"]["status"] == 1).nonzero()[:, 0]
    depth_t = torch.zeros(R, device=backend).index_put((hit,), ret["rendered"]["depth_volume"])
    mask_t = torch.zeros(R, device=backend).index_put((hit,), ret["rendered"]["mask_volume"])
    sel = getattr(model, "_rays_sel", None)
    dv, mv = vol["rendered"]["depth_volume"], vol["rendered"]["mask_volume"]
    if dv.shape[0] != R:
        rows = tested["rays_inds"].new_tensor([], dtype=torch.long) if sel is None else sel
        dv = torch.zeros(R, device=backend).index_put((rows,), dv)
        mv = torch.zeros(R, device=backend).index_put((rows,), mv)
    both = (mask_t > 0.5) & (mv > 0.5)
    err = (depth_t - dv.detach()).abs()[both] / MARCH["step_size"]
    print(f"depth difference on {int(both.sum())} rays: max {float(err.max()):.3f} march steps")
    assert int(both.sum()) > 100
    assert float(err.max()) <= 0.54


def test_edge_cases(backend):
    p, model, o, d, _, _ = _scene(backend, "f32", N=128)
    tested = model.ray_test(o, d, near=0.01, far=None)
    R = tested["num_rays"]
    occ_val = model.accel.occ_val.clone()
    # a ray that starts inside the surface (in an occupied voxel: step 1 comes first) hits at near
    model.accel.set_all_occupied()
    oi = torch.zeros(8, 3, device=backend) + torch.linspace(-0.1, 0.1, 8, device=backend)[:, None]
    di = torch.nn.functional.normalize(torch.ones(8, 3, device=backend), dim=-1)
    t_in = model.ray_test(oi.contiguous(), di.contiguous(), near=0.01, far=None)
    r_in = model.ray_query(ray_tested=t_in, config=_cfg(), return_details=True)
    assert bool((r_in["details"]["status"] == 1).all()) and bool((r_in["details"]["n_steps"] == 1).all())
    assert torch.equal(r_in["details"]["t"], t_in["near"])
    model.accel.occ_val.copy_(occ_val)
    model.accel.pack_bits()
    # max_march_iters = 1: a ray that does not hit on its first query is ALIVE
    r1 = model.ray_query(ray_tested=tested, config=_cfg(max_march_iters=1), return_details=True)["details"]
    full = model.ray_query(ray_tested=tested, config=_cfg(), return_details=True)["details"]
    queried = r1["n_steps"] == 1
    assert int(queried.sum()) > 20 and bool((r1["status"][queried] != 2).all())
    assert bool((r1["status"][queried & (full["n_steps"] > 1)] == 0).all()) and int((r1["status"] == 0).sum()) > 20
    assert bool((r1["n_steps"] <= 1).all())
    # far in front of the surface: OUT
    hit = full["status"] == 1
    short = dict(tested, far=torch.where(hit, full["t"] - 0.05, tested["far"]).contiguous())
    rs = model.ray_query(ray_tested=short, config=_cfg(), return_details=True)
    assert bool((rs["details"]["status"][hit] == 2).all()) and rs["volume_buffer"]["type"] == "empty"
    # an all-empty occupancy grid: every ray OUT without a query
    model.accel.occ_val.zero_()
    model.accel.pack_bits()
    re_ = model.ray_query(ray_tested=tested, config=_cfg(), return_details=True)
    assert re_["volume_buffer"]["type"] == "empty"
    assert bool((re_["details"]["status"] == 2).all()) and bool((re_["details"]["n_steps"] == 0).all()) and R > 0
    # scheduling keys of the CUDA implementation that would change results, and unknown modes, raise by name
    with pytest.raises(NotImplementedError, match="drop_alive_rate"):
        model.ray_query(ray_tested=tested, config=_cfg(drop_alive_rate=0.1))
    with pytest.raises(NotImplementedError, match="tail_sample_step_size"):
        model.ray_query(ray_tested=tested, config=_cfg(tail_sample_step_size=0.01))
    with pytest.raises(ValueError, match="query_mode"):
        model.ray_query(ray_tested=tested, config=dict(_cfg(), query_mode="march_occ"))


def test_other_models_refuse_the_mode():
    from neuralsim_amd.fields.batched_neus import BatchedLoTDNeuSModel
    from neuralsim_amd.fields.neus import LoTDNeuSModel
    from neuralsim_amd.fields.permuto_neus import PermutoNeuSModel
    assert LoTDNeuSModel._sphere_trace_ok and not PermutoNeuSModel._sphere_trace_ok and not BatchedLoTDNeuSModel._sphere_trace_ok
    m = object.__new__(PermutoNeuSModel)
    with pytest.raises(NotImplementedError, match="query_mode='sphere_trace'"):
        LoTDNeuSModel._ray_query_sphere_trace(m, None, dict(num_rays=0), {}, dict(PRESET), False, False)


def test_renderer_with_bypass_ray_query_cfg(backend):
    """``renderer.render(..., bypass_ray_query_cfg={class_name: {query_mode: sphere_trace, query_param: ...}})`` (inspect_rendering.py:
    101-109): the four images over all rays, finite, opaque exactly on the hit rays."""
    from neuralsim_amd.renderers.single_volume_renderer import SingleVolumeRenderer
    _, model, o, d, h, _ = _scene(backend, "fp16", N=256)
    model.ray_query_cfg = dict(query_mode="march_occ_multi_upsample", query_param=dict(QP_VOLUME))
    r = SingleVolumeRenderer(dict(with_rgb=True, with_normal=True, near=0.01, depth_use_normalized_vw=True, perturb=False)).eval()
    bypass = dict(Main=dict(query_mode="sphere_trace", query_param=dict(PRESET)))
    out = r.render(model, rays=[o, d], rays_h_appear=h, bypass_ray_query_cfg=bypass, render_per_obj_individual=True,
                   return_details=True, return_buffer=True)
    img = out["rendered"]
    N = o.shape[0]
    for k, sh in (("rgb_volume", (N, 3)), ("depth_volume", (N,)), ("mask_volume", (N,)), ("normals_volume", (N, 3))):
        assert img[k].shape == sh and bool(torch.isfinite(img[k]).all()), k
    det = out["raw_per_obj_model"]["main"]["details"]
    hit_rays = out["raw_per_obj_model"]["main"]["volume_buffer"]["rays_inds_hit"]
    assert int((det["status"] == 1).sum()) == hit_rays.shape[0] > 50
    want = torch.zeros(N, device=backend).index_put((hit_rays,), torch.ones(hit_rays.shape[0], device=backend))
    assert torch.equal(img["mask_volume"], want)
    assert bool((img["depth_volume"][hit_rays] > 2.0).all()) and float(img["normals_volume"][hit_rays].norm(dim=-1).min()) > 0.9
    # the same call volume-renders without the bypass: many samples per ray
    vol = r.render(model, rays=[o, d], rays_h_appear=h, return_buffer=True)
    assert int(vol["volume_buffer"]["pack_infos_hit"][:, 1].max()) > 1


@needs_reference
def test_reference_renderer_drives_the_mode(backend):
    """The reference's own ``SingleVolumeRenderer`` with the call of inspect_rendering.py:101-109 (``bypass_ray_query_cfg`` keyed
    by the object's class name, ``render_per_obj_individual``, ``only_cr``) on this model: its images are the tracer's."""
    from renderer_scenario import build_scenario
    sc = build_scenario("main_train", backend)
    bypass = {"Main": dict(query_mode="sphere_trace", query_param=dict(PRESET))}
    with ref_glue.reference_renderer_modules() as mods:
        scene = ref_glue.FakeScene(backend, image_embeddings=ref_glue.FixedEmbeddings(sc["h_appear"]),
                                   convert_rays_in_node=mods.get("convert_rays_in_node"))
        scene.add(ref_glue.FakeNode(sc["model"], "Main", "main"))
        r = ref_glue.make_reference_renderer(mods, dict(sc["common"], with_normal=True), training=False)
        cam = mods["classes"]["Camera"]("cam0")
        with torch.no_grad():
            ret = r.ray_query(sc["rays_o"], sc["rays_d"], rays_ts=torch.zeros(sc["N"], device=backend), scene=scene, observer=cam,
                              return_buffer=True, return_details=True, render_per_obj_individual=True, only_cr=True,
                              bypass_ray_query_cfg=bypass)
    raw = ret["raw_per_obj_model"]["main"]
    vb = raw["volume_buffer"]
    assert vb["type"] == "packed" and bool((vb["pack_infos_hit"][:, 1] == 1).all()) and bool((vb["opacity_alpha"] == 1).all())
    N = sc["N"]
    img = ret["rendered"]
    for k in ("rgb_volume", "depth_volume", "mask_volume"):
        assert img[k].shape[0] == N and bool(torch.isfinite(img[k]).all()), k
    want = torch.zeros(N, device=backend).index_put((vb["rays_inds_hit"],), torch.ones(vb["t"].shape[0], device=backend))
    assert torch.allclose(img["mask_volume"], want, atol=1e-6) and int(want.sum()) > 5
    assert torch.allclose(img["depth_volume"][vb["rays_inds_hit"]], vb["t"], atol=1e-5)
    assert ret["rendered_per_obj"]["main"]["mask_volume"].shape == (N,)
