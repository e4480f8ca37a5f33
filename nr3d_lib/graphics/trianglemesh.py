"""``nr3d_lib.graphics.trianglemesh`` (reference imports: code_single/tools/extract_mesh.py:26, code_multi/tools/extract_mesh.py):
``extract_mesh`` runs on this package's marching cubes (neuralsim_amd/mesh.py)."""
from neuralsim_amd.mesh import extract_mesh  # noqa: F401
