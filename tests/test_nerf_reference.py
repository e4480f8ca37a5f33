"""The reference's own sources on top of the close-range LoTD NeRF model (neuralsim_amd/fields/nerf.py) through the nr3d_lib
shim: the ``LoTDNeRFObj`` / ``LoTDNeRFStreet`` wrappers (app/models/single/nerf.py:33-143), ``SingleVolumeRenderer``
(app/renderers/single_volume_renderer.py) with the model as the close-range object -- alone and with the distant model and
the sky behind it -- against an integration of the restatement's buffer (tests/nerf_ref.py), and ``SparsityLoss`` /
``LidarLoss`` (app/loss/sparsity.py, lidar.py) on the returned buffers.  Emulator backend only; the renderer outputs of one
scene are frozen in tests/golden/nerf_renderer_fixture.npz and replayed by tests/test_nerf.py where the reference is absent."""
import os
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import nerf_ref as nr
import ref_glue
import test_nerf as T
from oracle import distant as od, pack_ops as opo, render as orr, sky as osky
from renderer_scenario import run_reference

needs_reference = ref_glue.needs_reference(ref_glue.reference_available(), reason="executes the reference's own sources (emulator backend); replayed from tests/golden/nerf_renderer_fixture.npz by tests/test_nerf.py")
GOLDEN = Path(__file__).resolve().parent / "golden" / "nerf_renderer_fixture.npz"


def restatement_images(sc, distant, sky):
    """rgb / depth / mask [N] of the scene from the restatement's buffer (its own march), merged with the oracle's distant
    shells and blended with the oracle's sky."""
    r, p = T.rays(), sc["p"]
    o, d, hit, ha = r["o"], r["d"], r["hit"], r["ha"]
    hidx = hit.nonzero()[:, 0]
    with torch.no_grad():
        q = nr.query_at(p, o[hit], d[hit], r["t"], r["ridx"], T.STEP, ha[hit])
        pi = torch.stack([torch.cumsum(r["counts"], 0) - r["counts"], r["counts"]], dim=-1)
        if not distant:
            vi = orr.volume_integration(q["opacity_alpha"], r["t"], q["rgb"], None, pi, False)
            out = {}
            for k in ("rgb_volume", "depth_volume", "mask_volume"):
                full = torch.zeros([T.N, *vi[k].shape[1:]])
                full[hidx] = vi[k]
                out[k] = full
        else:
            _, far, _ = orr.aabb_ray_test(o, d, T.AABB[0], T.AABB[1], 0.01, None)
            near_dv = torch.where(hit, far, torch.full_like(far, 0.01))
            K = 16
            dvo = od.distant_ray_query(sc["pd"], o, d, near_dv, ha, T.AABB[0], T.AABB[1], K=K)
            pi_dv = opo.get_pack_infos_from_n(torch.full((T.N,), K))
            keep = r["counts"] > 0
            pidx_dv, pidx_cr, pi_tot = opo.merge_two_packs_sorted(dvo["t"].flatten(), pi_dv, torch.arange(T.N), r["t"], pi[keep],
                                                                   hidx[keep])
            S = T.N * K + r["t"].shape[0]
            tt, aa, cc = torch.zeros(S), torch.zeros(S), torch.zeros(S, 3)
            tt[pidx_dv], tt[pidx_cr] = dvo["t"].flatten(), r["t"]
            aa[pidx_dv], aa[pidx_cr] = dvo["opacity_alpha"].flatten(), q["opacity_alpha"]
            cc[pidx_dv], cc[pidx_cr] = dvo["rgb"].flatten(0, 1), q["rgb"]
            out = orr.volume_integration(aa, tt, cc, None, pi_tot, False)
        if sky:
            ws, bs = osky.make_sky_params(10, 4, seed=21)
            rgb_sky = osky.sky_forward(torch.nn.functional.normalize(d, dim=-1), ha, ws, bs)
            out = dict(out, rgb_volume=osky.blend_sky(out["rgb_volume"], out["mask_volume"], rgb_sky))
    return {k: out[k] for k in ("rgb_volume", "depth_volume", "mask_volume")}


@needs_reference
@pytest.mark.parametrize("behind", [False, True])
def test_reference_renderer_renders_the_nerf_model(backend, behind):
    """The reference's SingleVolumeRenderer with the model as the close-range object, alone | with the distant model and the
    sky behind it: the buffer without ``nablas`` (``with_normal: true`` in the yaml), hit-only packs, the images."""
    sc = T.scene(backend, distant=behind, sky=behind)
    with ref_glue.reference_renderer_modules() as mods:
        got = run_reference(mods, sc, backward=True)
    want = restatement_images(sc, behind, behind)
    for k, w in want.items():
        e = float((got["rendered"][k] - w).abs().max())
        print(f"[nerf reference renderer behind={behind}] {k} {e:.3e}")
        assert e < (2e-2 if k == "depth_volume" else 3e-4), (k, e)
    assert float(got["grads"]["main.encoding.flattened_params"].abs().sum()) > 0 and "main.rad_w" in got["grads"]
    if behind:
        assert float(got["rendered"]["mask_volume"].min()) > 0.99
        if os.environ.get("NSIM_WRITE_GOLDEN") == "1":
            np.savez(str(GOLDEN), **{k: v.numpy() for k, v in got["rendered"].items() if k in want},
                     samples_cnt=got["samples_cnt"].numpy())
        fx = np.load(str(GOLDEN))
        for k in want:      # the committed fixture is what this run produces
            assert float(np.abs(fx[k] - got["rendered"][k].numpy()).max()) < 1e-5, k


class _Tf:
    def forward(self, x, inv=False):
        return x

    def vec_3(self):
        return torch.ones(3)


@needs_reference
def test_reference_wrappers_load_over_the_shim_class():
    """``LoTDNeRFObj`` / ``LoTDNeRFStreet`` derive from the shim's class unchanged; ``asset_populate`` hands the cubic /
    cuboid AABB of ``populate_cfg.use_cuboid`` to ``populate``."""
    from neuralsim_amd.fields.nerf import LoTDNeRFModel
    pts = torch.tensor([[-2.0, -1.0, -0.5], [2.0, 1.0, 0.5], [0.0, 0.3, 0.1]])
    scene = SimpleNamespace(process_observer_infos=lambda far_clip: SimpleNamespace(all_frustum_pts=pts),
                            frozen_at_global_frame=lambda i: None, unfrozen=lambda: None, id="scene0")
    obj = SimpleNamespace(world_transform=_Tf(), scale=_Tf(), id="street", class_name="Street")
    with ref_glue.reference_model_wrapper_modules() as mods:
        nerf = mods["app.models.single.nerf"]
        assert issubclass(nerf.LoTDNeRFObj, LoTDNeRFModel) and issubclass(nerf.LoTDNeRFStreet, LoTDNeRFModel)
        m = nerf.LoTDNeRFObj(**T.yaml_params(6, 0))
        m.asset_populate(scene=scene, obj=obj, config={}, device=torch.device("cpu"))
        assert torch.equal(m.space.aabb.cpu(), T.AABB) and m.asset_training_initialize(scene, obj, {}) is False
        assert "LoTDNeRFObj#Street" in nerf.LoTDNeRFObj.asset_compute_id(scene=scene, obj=obj)
        st = nerf.LoTDNeRFStreet(**T.yaml_params(6, 0))
        st.asset_populate(scene=scene, obj=obj, config=dict(extend_size=10.0, use_cuboid=False), device=torch.device("cpu"))
        assert torch.equal(st.space.aabb.cpu(), torch.tensor([[-2.0, -2.0, -2.0], [2.0, 2.0, 2.0]]))
        assert st.encoding.cfg.lod_res3[0] == [4, 4, 4]
        enc = dict(T.yaml_params()["encoding_cfg"], lotd_use_cuboid=True)
        sc = nerf.LoTDNeRFStreet(**T.yaml_params(6, 0, encoding_cfg=enc))
        sc.asset_populate(scene=scene, obj=obj, config=dict(extend_size=10.0, use_cuboid=True), device=torch.device("cpu"))
        assert torch.equal(sc.space.aabb.cpu(), torch.stack([pts[0], pts[1]])) and sc.encoding.cfg.lod_res3[0] == [16, 8, 4]
        assert st.ray_query_cfg.query_mode == "march_occ"


@needs_reference
def test_reference_sparsity_and_lidar_losses(backend):
    """``SparsityLoss{type: density_reg, key: sigma}`` on ``sample_pts_uniform`` and ``LidarLoss{depth, line_of_sight{fn_type:
    nerf}}`` on a ``with_rgb=False`` render of the reference's renderer: finite values, gradients into the table, none into the
    radiance decoder."""
    from nr3d_lib.config import ConfigDict
    sc = T.scene(backend, distant=False, sky=False)
    sc["common"] = dict(sc["common"], with_rgb=False, with_normal=False, depth_use_normalized_vw=True)
    m = sc["model"]
    with ref_glue.reference_renderer_modules() as mods:
        scene = ref_glue.FakeScene(backend, main_class_name="Main", image_embeddings=ref_glue.FixedEmbeddings(sc["h_appear"]))
        scene.add(ref_glue.FakeNode(m, "Main", "main"))
        rr = ref_glue.make_reference_renderer(mods, sc["common"], training=True)
        ret = rr.ray_query(sc["rays_o"], sc["rays_d"], rays_ts=torch.zeros(T.N, device=backend), scene=scene,
                           observer=mods["classes"]["Camera"]("lidar0"), return_buffer=True, return_details=True)
    assert "rgb" not in ret["volume_buffer"] and "rgb_volume" not in ret["rendered"] and "nablas" not in ret["volume_buffer"]
    g = torch.Generator().manual_seed(8)
    ranges = (ret["rendered"]["depth_volume"].detach().cpu() + torch.randn(T.N, generator=g) * 0.05).clamp_min(0.1).to(backend)
    with ref_glue.reference_lidar_loss_module() as lidar:
        ll = lidar.LidarLoss(depth=dict(w=1.0, fn_type="l1"), line_of_sight=dict(w=0.5, fn_type="nerf", fn_param=dict(sigma=0.1)),
                             discard_outliers_median=0)     # (the harness's l1_loss stand-in has no reduction="none")
        losses = dict(ll(None, ret, None, dict(ranges=ranges), it=0, far=10.0))
    assert {"lidar_loss.depth", "lidar_loss.los.neighbor", "lidar_loss.los.empty"} <= set(losses)
    with ref_glue.reference_loss_module("sparsity") as sp:
        loss_fn = sp.SparsityLoss(class_name_cfgs=ConfigDict(Main=ConfigDict(w=1.0e-3, key="sigma", type="density_reg", lamb=0.05)))
        scene.asset_bank = {ret["raw_per_obj_model"]["main"]["model_id"]: m}
        us = dict(Main=m.sample_pts_uniform(65, generator=torch.Generator(device=backend).manual_seed(1)))
        losses.update(loss_fn(scene, ret, us, None, None, it=0))
    assert "loss_sparsity.Main" in losses and all(bool(torch.isfinite(v)) for v in losses.values())
    for k in ("lidar_loss.los.empty", "loss_sparsity.Main"):
        for q in m.parameters():
            q.grad = None
        losses[k].backward(retain_graph=True)
        assert float(m.encoding.flattened_params.grad.abs().sum()) > 0 and float(m.den_w.grad.abs().sum()) > 0, k
        assert m.rad_w.grad is None or float(m.rad_w.grad.abs().sum()) == 0.0
