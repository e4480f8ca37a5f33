"""Generate tests/golden/segmentation_fixture.pt: the instance / class segmentation of the REFERENCE's own
``BufferComposeRenderer`` source (app/renderers/buffer_compose_renderer.py:182-188, 268-311, 549-572, loaded unchanged by
tests/ref_glue.py) driving this repository's models on the multi-object scenario of tests/compose_scenario.py, with
``render_per_obj_individual=True`` and ``segmentation_threshold = 0.002``.

Runs in the authoring container only (needs the reference's sources; the kernels run on the test-only emulator build of the
same .hip sources).  Data only: the two buffers, every object's individual ``mask_volume`` / ``depth_volume``, the index maps.
``tests/test_segmentation.py::test_segmentation_matches_the_frozen_reference`` replays the native renderer against it on both
backends.   python tests/golden/make_segmentation_fixture.py
"""
import ctypes
import sys
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "tests" / "emu")]

import build_emu  # noqa: E402
import ref_glue  # noqa: E402
from neuralsim_amd import _lib  # noqa: E402
from segmentation_ref import ambiguous_rays  # noqa: E402
from test_segmentation import DEPTH_TOL, MASK_TOL, MAX_LEFT_OUT, SEG_THR  # noqa: E402


def main():
    assert ref_glue.reference_available(), "needs the reference's sources"
    lib = _lib.bind(ctypes.CDLL(str(build_emu.build())))
    _lib.get_lib = lambda: lib                      # the emulator backend, as tests/conftest.py installs it
    _lib.stream_handle = lambda: 0
    _lib.require_device = lambda t, name="tensor": None
    import compose_scenario as cs
    dev = torch.device("cpu")
    sc = cs.build(dev)
    with ref_glue.reference_compose_renderer_modules() as mods:
        from nr3d_lib.config import ConfigDict
        AA = mods["AssetAssignment"]
        main_m, mb, sky = sc["main"], sc["vehicle"], sc["sky"]
        main_m.assigned_to, main_m.is_ray_query_supported, main_m.is_batched_query_supported = AA.OBJECT, True, False
        mb.assigned_to, mb.is_ray_query_supported = AA.MULTI_OBJ, True
        sky.assigned_to, sky.is_ray_query_supported = AA.SCENE, False
        scene = ref_glue.FakeComposeScene(dev, mods["Scene"], image_embeddings=ref_glue.FixedEmbeddings(sc["h_appear"]))
        scene.add(ref_glue.FakeNode(main_m, "Main", "main", ref_glue.FakeTransform(device=dev)))
        for k, (R, t, s) in sc["poses"].items():
            scene.add(ref_glue.FakeNode(mb, "Vehicle", k, ref_glue.FakeTransform(R, t, s, device=dev)))
        scene.add(ref_glue.FakeNode(sky, "Sky", "sky", ref_glue.FakeTransform(device=dev)))
        rr = mods["compose"].BufferComposeRenderer(ConfigDict(common=ConfigDict(dict(sc["common"], segmentation_threshold=SEG_THR)),
                                                              train=ConfigDict(), val=ConfigDict()))
        rr.image_postprocessor = None
        rr.eval()
        obs = type("Camera", (mods["classes"]["Camera"], ref_glue.FakeObserver), {})("cam0")
        with torch.no_grad():
            ret = rr.ray_query(sc["rays_o"], sc["rays_d"], rays_ts=torch.zeros(sc["N"], device=dev), scene=scene, observer=obs,
                               render_per_obj_individual=True)
        ins_map, cls_map = scene.get_drawable_instance_ind_map(), scene.get_drawable_class_ind_map()
    N = sc["N"]
    own = lambda v: v.detach().cpu().clone().contiguous()          # noqa: E731  (torch.save writes whole storages)
    out = dict(segmentation_threshold=SEG_THR, N=N,
               ins_seg_mask_buffer=own(ret["ins_seg_mask_buffer"]), class_seg_mask_buffer=own(ret["class_seg_mask_buffer"]),
               per_obj={oid: dict(mask_volume=own(r["mask_volume"]), depth_volume=own(r["depth_volume"]))
                        for oid, r in ret["rendered_per_obj"].items()},
               instance_ind_map={k: int(v) for k, v in ins_map.items()}, class_ind_map={k: int(v) for k, v in cls_map.items()})
    # a fixture that hides the comparison cannot be produced: the rays the test may leave out stay within its cap, and the
    # overlap of the two vehicles is among the rays that remain
    amb = ambiguous_rays(out["per_obj"], SEG_THR, MASK_TOL, DEPTH_TOL)
    assert int(amb.sum()) <= MAX_LEFT_OUT * N, f"{int(amb.sum())} of {N} rays are ambiguous"
    po = out["per_obj"]
    both = (po["car0"]["mask_volume"] > SEG_THR) & (po["car2"]["mask_volume"] > SEG_THR)
    assert int((both & ~amb).sum()) > 0, "no unambiguous ray on which both vehicles qualify"
    kept = set(out["ins_seg_mask_buffer"][~amb].tolist())
    assert {-1, ins_map["main"], ins_map["car0"], ins_map["car2"]} <= kept, kept
    torch.save(out, HERE / "segmentation_fixture.pt")
    print("wrote", HERE / "segmentation_fixture.pt", (HERE / "segmentation_fixture.pt").stat().st_size, "bytes;",
          "ambiguous rays:", int(amb.sum()), "overlap rays kept:", int((both & ~amb).sum()), "instances:", sorted(kept))


if __name__ == "__main__":
    main()
