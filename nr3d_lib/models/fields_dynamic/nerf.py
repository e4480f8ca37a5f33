"""``nr3d_lib.models.fields_dynamic.nerf`` (reference import: app/models/single/dynamic_nerf.py:18).

``EmerNeRFOnlyDynamicModel`` is the real class behind the reference's constructor keywords
(neuralsim_amd/fields/dynamic_nerf.py); the full ``EmerNeRFModel`` (static + dynamic branches) is not built."""
from neuralsim_amd.fields.dynamic_nerf import EmerNeRFOnlyDynamicModel  # noqa: F401


class EmerNeRFModel:
    def __init__(self, *a, **k):
        raise NotImplementedError("EmerNeRFModel (static + dynamic branches, flow field, shadow head) is not built; the "
                                  "dynamic-only EmerNeRFOnlyDynamicModel is")
