"""Generate tests/golden/street_loss_fixture.pt: what the REFERENCE's own ``MaskOccupancyLoss``, ``MaskEntropyRegLoss.
forward_code_single``, ``SparsityLoss``, ``ClearanceLoss`` and ``LidarLoss`` (app/loss/{mask, mask_entropy, sparsity, clearance,
lidar}.py, loaded unchanged by ``ref_glue.reference_loss_module``) return on the inputs of tests/test_street_losses.py
(``fixture_inputs``) -- the shim's pack ops and elementwise losses on the emulator backend underneath, small stand-ins for the
scene objects the classes look things up in -- together with the inputs: losses, gradients, the error map of the mask loss and
the final mask of the lidar loss.  Data only, float32 as the reference ran it.  The replay (tests/test_street_losses.py::
test_reference_classes_replayed_from_the_fixture) runs on both backends where the reference tree is absent.

Where the reference tree is readable:   python tests/golden/make_street_loss_fixture.py"""
import ctypes
import sys
import types
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "tests" / "emu")]

import build_emu  # noqa: E402
import ref_glue  # noqa: E402
import test_street_losses as t  # noqa: E402
from neuralsim_amd import _lib  # noqa: E402
from util import leaf  # noqa: E402

DEV = torch.device("cpu")


def fake_scene():
    """what the loss classes touch of a Scene: the device, the main class name, one drawable per class, the asset bank"""
    node = lambda i: types.SimpleNamespace(id=i)      # noqa: E731
    return types.SimpleNamespace(device=DEV, main_class_name="Street",
                                 drawable_groups_by_class_name=dict(Street=[node("street0")], Distant=[node("distant0")]),
                                 asset_bank={"street_model": object(), "distant_model": object()})


def raw_per_obj(cr_vb, dv_vb=None, details=None):
    raw = {"street0": dict(volume_buffer=cr_vb, class_name="Street", model_id="street_model", details=details or {})}
    if dv_vb is not None:
        raw["distant0"] = dict(volume_buffer=dv_vb, class_name="Distant", model_id="distant_model", details={})
    return raw


def freeze(losses, leaves, **extra):
    """backward of sum(COEF_k loss_k) -- the upstream gradients the replay applies -- and everything detached"""
    tot = sum(c * v for c, v in zip(t.COEF, losses.values()))
    tot.backward()
    return dict(losses={k: v.detach().clone().reshape(()) for k, v in losses.items()},
                grads=[x.grad.clone() if x.grad is not None else torch.zeros_like(x) for x in leaves], **extra)


def main():
    lib = _lib.bind(ctypes.CDLL(str(build_emu.build())))
    _lib.get_lib, _lib.stream_handle, _lib.require_device = (lambda: lib), (lambda: 0), (lambda t, name="tensor": None)
    inp, out, scene = t.fixture_inputs(), {}, fake_scene()
    N = t.FIX_N
    with ref_glue.reference_loss_module("mask") as mod:
        for mode in (None, "always_occupied", "only_cull_non_occupied", "only_preserve_occupied"):
            pred = leaf(inp["mask_pred"])
            fn = mod.MaskOccupancyLoss(**t.FIX_MASK, special_mask_mode=mode)
            losses, err = fn(scene, dict(rendered=dict(mask_volume=pred)), {}, dict(image_occupancy_mask=inp["mask_gt"]), 0)
            out[f"mask.{mode}"] = freeze(losses, [pred], err=err.detach().clone())
    with ref_glue.reference_loss_module("mask_entropy") as mod:
        for name, cfg in t.FIX_ENTROPY.items():
            vcr, vdv = leaf(inp["cr"]["vw_in_total"]), leaf(inp["dv"]["vw_in_total"])
            ret = dict(rendered=dict(mask_volume=torch.zeros(N)),
                       raw_per_obj_model=raw_per_obj(dict(inp["cr"], vw_in_total=vcr), dict(inp["dv"], vw_in_total=vdv)))
            out[f"entropy.{name}"] = freeze(mod.MaskEntropyRegLoss(**cfg).forward_code_single(scene, ret, (N,), 0), [vcr, vdv])
    with ref_glue.reference_loss_module("sparsity") as mod:
        x = leaf(inp["sdf"])
        fn = mod.SparsityLoss(class_name_cfgs=dict(Street=dict(t.FIX_SPARSITY)))
        out["sparsity"] = freeze(fn(scene, dict(raw_per_obj_model=raw_per_obj(dict(type="packed"))), dict(Street=dict(sdf=x)), {}, {}, 0), [x])
    with ref_glue.reference_loss_module("clearance") as mod:
        x = leaf(inp["near_sdf"])
        fn = mod.ClearanceLoss(class_name_cfgs=dict(Street=dict(t.FIX_CLEARANCE)), drawable_class_names=["Street", "Distant"])
        losses = fn(scene, dict(raw_per_obj_model=raw_per_obj(dict(type="packed"), details=dict(near_sdf=x))), {}, {}, {}, 0, mode="pixel")
        out["clearance"] = freeze(losses, [x])
    with ref_glue.reference_loss_module("lidar") as mod:
        for case in ("lidar", "lidar_all_return"):
            c = inp[case]
            for name, cfg in t.FIX_LIDAR.items():
                d, vw = leaf(c["depth"]), leaf(c["vb"]["vw"])
                ret = dict(rendered=dict(depth_volume=d, mask_volume=c["mask"]), volume_buffer=dict(c["vb"], vw=vw))
                fn = mod.LidarLoss(**cfg)
                # the class keeps its final mask to itself: the same forward once more, up to the mask (lidar.py:264-284)
                losses = fn(scene, ret, {}, dict(ranges=c["ranges"]), it=0, far=None)
                mask = c["ranges"] <= fn.discard_toofar
                e = (d.detach() - c["ranges"]).abs() * mask
                mask = mask & ~(e > torch.sort(e).values[N // 2] * fn.discard_outliers_median)
                out[f"{case}.{name}"] = freeze(losses, [d, vw], keep=mask)
    path = HERE / "street_loss_fixture.pt"
    torch.save(dict(inputs=inp, outputs=out), path)
    for k, v in out.items():
        print(k, {n: float(x) for n, x in v["losses"].items()})
    print("bytes", path.stat().st_size)


if __name__ == "__main__":
    main()
