"""``nr3d_lib.models.grid_encodings.utils`` at the call the reference makes: ``voxel_verts(_0=-1., _1=1.)``
(code_single/tools/extract_occgrid.py:94), the 8 corners of a box -- the tool uses only their per-axis min and max."""
import torch


def voxel_verts(_0=0.0, _1=1.0) -> torch.Tensor:
    """[8, 3]: the corners of the box [_0, _1]^3 (x slowest)."""
    v = torch.tensor([_0, _1])
    return torch.stack(torch.meshgrid(v, v, v, indexing="ij"), dim=-1).view(8, 3)
