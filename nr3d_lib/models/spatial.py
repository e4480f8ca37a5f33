"""``nr3d_lib.models.spatial.AABBSpace`` (reference imports: app/models/asset_base.py:15, app/resources/nodes.py).
The block / forest spaces of the large-scene models are outside the hot path; ``ForestBlockSpace`` is an import-surface name
(code_single/tools/extract_mesh.py:25 imports it without using it)."""
from neuralsim_amd.spatial import AABBSpace  # noqa: F401


class ForestBlockSpace:
    def __init__(self, *a, **k):
        raise NotImplementedError("ForestBlockSpace: forest / block spaces of the large-scene models are not built here")
