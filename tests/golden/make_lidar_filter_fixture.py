"""Writes tests/golden/lidar_filter_fixture.pt: the reference's OWN ``MultiCamBundle.project_pts_in_image``
(app/resources/observers/cameras.py:397-446, 537-538) and ``SceneDataLoader._filter_lidar_gts`` (dataio/data_loader/
base_loader.py:732-844), loaded unchanged from the reference tree (authoring container only; ``ref_glue.REF_ROOT``) and run on
CPU attributes of this repository's ``nr3d_lib`` shim.  The loader method is called unbound with a minimal ``self`` (camera ids,
``config.tags``, ``get_image_ignore_mask``, device), in the manner of tests/test_nerf_reference.py; the cameras are plain objects
carrying the attributes ``MultiCamBundle`` reads off a frozen ``Camera`` node.

    python tests/golden/make_lidar_filter_fixture.py

The scene: 4000 world points in a +-60 m cube, ranges with zeros and negatives, 3 OpenCV cameras (skew, five coefficients; stored
at twice the trained size with ``downscale`` 2), per-camera ignore masks of different sizes, an AABB, box metas of three classes
over 8 data frames of which ``filter_out_obj_classnames`` selects two (6 boxes at the frozen frame + ``data_frame_offset``).
Stored: the inputs, the kept indices after each of the four stages, the projection tuple.  Data only."""
import math
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

N = 4000
HW_RAW = [(128, 192), (96, 160), (128, 192)]
DOWNSCALE = 2
DIST = [[-0.05, 0.01, 0.001, -0.0015, 0.0005], [0.0, 0.0, 0.0, 0.0, 0.0], [0.03, -0.004, -0.0008, 0.0012, 0.0002]]
FRAME, DATA_FRAME_OFFSET = 2, 3


def _rodrigues(ax, a):
    ax = ax / ax.norm()
    K = torch.tensor([[0.0, -ax[2], ax[1]], [ax[2], 0.0, -ax[0]], [-ax[1], ax[0], 0.0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)


def _pose(g, spread):
    R = _rodrigues(torch.randn(3, generator=g, dtype=torch.float64), float(torch.rand(1, generator=g)) * 2 * math.pi)
    t = (torch.rand(3, generator=g, dtype=torch.float64) * 2 - 1) * spread
    m = torch.eye(4, dtype=torch.float64)
    m[:3, :3], m[:3, 3] = R, t
    return m


def main():
    import ref_glue
    import run_reference_train as rrt
    assert ref_glue.reference_available(), "the reference tree is needed to write this fixture"
    sys.path.append(str(ref_glue.REF_ROOT))
    rrt._install_third_party_stubs()
    from app.resources.observers.cameras import MultiCamBundle
    from dataio.data_loader.base_loader import SceneDataLoader
    from nr3d_lib.config import ConfigDict
    from nr3d_lib.models.attributes import CameraMatrix3x3, OpenCVCameraMatHW, TransformMat4x4, make_vector

    g = torch.Generator().manual_seed(20240219)
    cams, c2ws, intrs, masks = [], [], [], {}
    for c, (H, W) in enumerate(HW_RAW):
        c2w = _pose(g, 1.5).float()
        fx = 0.45 * W
        K = torch.tensor([[fx, 1.4, W / 2 + 0.6], [0.0, 1.05 * fx, H / 2 - 0.4], [0.0, 0.0, 1.0]])
        intr = OpenCVCameraMatHW(mat=CameraMatrix3x3(K), H=torch.tensor(float(H)), W=torch.tensor(float(W)),
                                 distortion=make_vector(5)(torch.tensor(DIST[c])))
        cid = f"camera_{c}"
        cams.append(SimpleNamespace(id=cid, intr=intr, world_transform=TransformMat4x4(c2w), i_prefix=(), i_is_single=True, near=None,
                                    far=None, frustum=torch.zeros(6, 4), frame_global_ts=None, frame_global_fi=None,
                                    dtype=torch.float32, device=torch.device("cpu"), scene=None))
        c2ws.append(c2w)
        intrs.append(K)
        h, w = H // DOWNSCALE, W // DOWNSCALE
        mk = torch.zeros(h, w, dtype=torch.bool)                    # a few large rectangles: mask edges are rare
        mk[10:30, 20 + 3 * c:50] = True
        mk[40:, :15] = True
        masks[cid] = mk
    pts = ((torch.rand(N, 3, generator=g, dtype=torch.float64) * 2 - 1) * 60.0).float()
    ranges = torch.rand(N, generator=g) * 70 + 0.5
    pick = torch.rand(N, generator=g)
    ranges[pick < 0.08] = 0.0
    ranges[pick > 0.94] = -1.0
    data = dict(rays_o=torch.randn(N, 3, generator=g), rays_d=torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1),
                ranges=ranges, idx=torch.arange(N))
    aabb = torch.tensor([[-40.0, -45.0, -30.0], [45.0, 40.0, 35.0]])

    def boxes(n):
        rows = []
        for _ in range(n):
            m = _pose(g, 40.0)[:3]
            s = 6.0 + 24.0 * torch.rand(3, generator=g, dtype=torch.float64)
            rows.append(torch.cat([m.reshape(-1), s]).numpy())
        return np.stack(rows) if rows else np.empty([0, 15])
    per_frame = {cls: [boxes(k) for k in counts] for cls, counts in
                 (("Vehicle", [1, 0, 2, 3, 1, 4, 2, 0]), ("Pedestrian", [0, 1, 1, 0, 2, 2, 1, 1]), ("Sign", [2, 2, 2, 2, 2, 2, 2, 2]))}
    classnames = ["Vehicle", "Pedestrian", "Cyclist"]                # (a class without metas is skipped, base_loader.py:811-813)
    k = FRAME + DATA_FRAME_OFFSET
    used = np.concatenate([per_frame["Vehicle"][k], per_frame["Pedestrian"][k]], axis=0)
    assert used.shape == (6, 15)

    scene = SimpleNamespace(i=FRAME, id="scene0", observers={c.id: c for c in cams}, data_frame_offset=DATA_FRAME_OFFSET,
                            metas=dict(obj_box_list_per_frame=per_frame, obj_box_list_per_frame_dynamic_only={}))
    loader = SimpleNamespace(cam_id_list=[c.id for c in cams], device=torch.device("cpu"),
                             config=ConfigDict(tags=ConfigDict(camera=ConfigDict(downscale=DOWNSCALE), image_ignore_mask=ConfigDict())),
                             get_image_ignore_mask=lambda scene_id, cam_id, frame_ind, device: masks[cam_id])
    stages = dict(valid=dict(), cams=dict(filter_in_cams=True), aabb=dict(filter_in_cams=True, filter_in_aabb=aabb),
                  objs=dict(filter_in_cams=True, filter_in_aabb=aabb, filter_out_objs=True, filter_out_obj_classnames=classnames))
    kept = {}
    for name, kw in stages.items():
        out = SceneDataLoader._filter_lidar_gts(loader, dict(data), pts, scene, filter_valid=True, **kw)
        assert sorted(out) == sorted(data)
        kept[name] = out["idx"].clone()
        print(name, kept[name].numel())

    bundle = MultiCamBundle(cams)
    bundle.intr.set_downscale(DOWNSCALE)
    Hm = max(m.shape[0] for m in masks.values())
    Wm = max(m.shape[1] for m in masks.values())
    ign = torch.zeros(len(cams), Hm, Wm, dtype=torch.bool)
    for c, cam in enumerate(cams):
        ign[c, :masks[cam.id].shape[0], :masks[cam.id].shape[1]] = masks[cam.id]
    pj = bundle.project_pts_in_image(pts.view(1, -1, 3), ignore_mask=ign)
    assert torch.equal(pj.mask.any(0).nonzero()[:, 0], SceneDataLoader._filter_lidar_gts(
        loader, dict(data), pts, scene, filter_valid=False, filter_in_cams=True)["idx"])
    print("projections", pj.n, "per camera", pj.mask.sum(1).tolist())
    fx = dict(pts=pts, data={k_: v for k_, v in data.items() if k_ != "idx"},
              cam_c2w=torch.stack(c2ws), cam_intr_raw=torch.stack(intrs), cam_hw_raw=torch.tensor(HW_RAW), downscale=DOWNSCALE,
              cam_intr=bundle.intr.mat_3x3().clone(), cam_hw=torch.stack([bundle.intr.H, bundle.intr.W], dim=-1),
              cam_models=["opencv"] * len(cams), cam_dist=torch.tensor(DIST), ignore=ign, aabb=aabb,
              boxes=torch.tensor(used, dtype=torch.float), classnames=classnames, frame=FRAME, data_frame_offset=DATA_FRAME_OFFSET,
              kept=kept, proj=dict(mask=pj.mask, n=int(pj.n), i=pj.i, u=pj.u, v=pj.v, d=pj.d))
    torch.save(fx, str(HERE / "lidar_filter_fixture.pt"))
    print("wrote", HERE / "lidar_filter_fixture.pt", (HERE / "lidar_filter_fixture.pt").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
