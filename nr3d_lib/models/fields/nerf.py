"""``nr3d_lib.models.fields.nerf`` (reference import: app/models/single/nerf.py:26): ``LoTDNeRFModel`` is the close-range
LoTD NeRF of this package (InstantNGP + UrbanNeRF, waymo/ngp_withlidar.230814.yaml); ``NeRFModel`` (a positional-encoding
MLP) is not on any hot path -- an importable name only."""
from neuralsim_amd.fields.nerf import LoTDNeRFModel  # noqa: F401

from .neus import _NotOnTheHotPath


class NeRFModel(_NotOnTheHotPath):
    pass
