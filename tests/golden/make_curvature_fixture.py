"""Generate tests/golden/curvature_fixture.pt: the scalar the REFERENCE's own ``SDFCurvatureRegLoss`` (app/loss/sdf_curvature.py,
loaded unchanged by tests/ref_glue.py) returns on the scene of tests/curvature_ref.py -- this package's model on the emulator
backend, ``ray_query`` with ``with_net_x`` -- together with everything the run drew: the model's weights, the rays, the tangent
directions of ``get_sdf_curvature_1d``.  Data only.  The replay (tests/test_curvature.py::
test_reference_class_scalar_replayed_from_the_fixture) runs on both backends where the reference tree is absent.

Where the reference tree is readable:   python tests/golden/make_curvature_fixture.py"""
import ctypes
import sys
import types
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "tests" / "emu")]

import build_emu  # noqa: E402
import curvature_ref as cref  # noqa: E402
import ref_glue  # noqa: E402
from neuralsim_amd import _lib  # noqa: E402


def main():
    lib = _lib.bind(ctypes.CDLL(str(build_emu.build())))
    _lib.get_lib, _lib.stream_handle, _lib.require_device = (lambda: lib), (lambda: 0), (lambda t, name="tensor": None)
    dev = torch.device("cpu")
    m, o, d = cref.scene_model(dev)
    _, q = cref.scene_query(m, o, d, with_net_x=True)
    vb = q["volume_buffer"]
    ret = dict(raw_per_obj_model=dict(main=dict(volume_buffer=vb, class_name="Main", model_id="main")))
    scene = types.SimpleNamespace(asset_bank=dict(main=m))
    with ref_glue.reference_loss_module("sdf_curvature") as mod:
        loss_mod = mod.SDFCurvatureRegLoss({"Main": {"w": cref.SCENE_W, "alpha_loss_on_render": cref.SCENE_ALPHA}}, ["Main"],
                                           on_uniform_samples=False, eps=cref.SCENE_EPS)
        torch.manual_seed(cref.SCENE_SEED)
        out = loss_mod(scene, ret, {}, {}, {}, 0)
    torch.manual_seed(cref.SCENE_SEED)
    dirs = torch.randn(vb["t"].shape[0], 3)
    table = m.encoding.flattened_params.detach()
    assert torch.equal(table.half().float(), table)              # fp16-representable: stored as fp16
    fx = dict(table=table.half(), sdf_w=m.sdf_w.detach().clone(), sdf_b=m.sdf_b.detach().clone(), rays_o=o.clone(), rays_d=d.clone(),
              dirs=dirs, eps=cref.SCENE_EPS, w=cref.SCENE_W * cref.SCENE_ALPHA,
              loss=out["loss_sdf_curvature_reg.Main.render"].detach().clone())
    torch.save(fx, HERE / "curvature_fixture.pt")
    print("samples", int(vb["t"].shape[0]), "loss", float(fx["loss"]), "bytes", (HERE / "curvature_fixture.pt").stat().st_size)


if __name__ == "__main__":
    main()
