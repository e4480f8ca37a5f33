"""Generate tests/golden/visible_grid_fixture.pt: recorded inputs and outputs of the reference's own ``VisibleGrid``
(app/visible_grid.py, source unchanged, loaded by tests/visible_grid_ref.py with stand-in modules: one block over [0, 1]^3, a bool
occupancy grid) at octree depth 5 -- the points, the reduced voxels with their hit counts, the voxels after
``postprocess(op)`` for the three operations, and the state dict its ``save`` writes.  Data only (tensors, ints, strings).
tests/test_visible_grid.py replays it on both backends.  Run from the repo root where the reference is readable:
    python tests/golden/make_visible_grid_fixture.py
"""
import sys
import tempfile
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import visible_grid_ref as vref

DEPTH = 5


def points():
    """a few hundred points of [0, 1]^3: a bent sheet (a surface seen by cameras), clusters in the 8 corner voxels and on the
    lower faces, repeated points (hit counts above 1), and some outside the box"""
    g = torch.Generator().manual_seed(20240219)
    u = torch.rand([260, 2], generator=g)
    sheet = torch.stack([u[:, 0], u[:, 1], 0.5 + 0.3 * torch.sin(3.0 * u[:, 0]) * torch.cos(2.0 * u[:, 1])], dim=-1)
    c = torch.tensor([0.004, 0.996])
    corners = torch.stack(torch.meshgrid(c, c, c, indexing="ij"), dim=-1).view(8, 3)
    faces = torch.rand([24, 3], generator=g)
    faces[:8, 0], faces[8:16, 1], faces[16:, 2] = 0.0, 0.0, 0.0
    outside = torch.rand([16, 3], generator=g) * 3.0 - 1.0
    outside[:, 0] = torch.where(outside[:, 0].abs() < 1.0, outside[:, 0] + 1.5, outside[:, 0])
    return torch.cat([sheet, sheet[:40], corners, corners[:3], faces, outside]).float().contiguous()


def main():
    pts = points()
    out = dict(octree_depth=DEPTH, aabb=torch.tensor([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]), pts=pts, post={})
    with tempfile.TemporaryDirectory() as tmp:
        for op in ("dilation", "close", "close2"):
            file = str(Path(tmp) / f"{op}.pt")
            voxels, hits, post = vref.run_reference(pts, DEPTH, op, save_to=file)
            out["voxels"], out["hits"] = voxels, hits
            out["post"][op] = post
            if op == "close":
                out["saved_state"] = torch.load(file, weights_only=False)
    torch.save(out, str(Path(__file__).with_name("visible_grid_fixture.pt")))
    print("wrote visible_grid_fixture.pt:", pts.shape[0], "points,", out["voxels"].shape[0], "voxels,",
          {k: int(v.shape[0]) for k, v in out["post"].items()})


if __name__ == "__main__":
    main()
