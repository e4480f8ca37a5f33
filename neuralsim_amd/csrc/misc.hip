// misc.hip -- version / error strings of the C ABI, and marching cubes on slabs of SDF lattices (nsim_mc_*).
#include "nsim_common.h"

// ------------------------------------------------------------------------------------------------ marching cubes
// nr3d_lib.graphics.trianglemesh.extract_mesh (code_single/tools/extract_mesh.py:124), the kernels behind neuralsim_amd/mesh.py.
//
// Input: one z-slab of a lattice of values, f32 [nzs + 1][ny][nx] (x fastest), lattice point (i, j, k) at
// bmin + h (i, j, k0 + k); optional single planes below / above the slab (central differences of the normals across slab
// borders).  Conventions (pinned by tests/test_mesh.py against the numpy restatement tests/mesh_ref.py):
//   * table: corner c is inside when its value is < level (case bit c); corners (0,0,0) (1,0,0) (1,1,0) (0,1,0) (0,0,1)
//     (1,0,1) (1,1,1) (0,1,1), edges 0-1 1-2 2-3 3-0 4-5 5-6 6-7 7-4 0-4 1-5 2-6 3-7.  Every ambiguous face is resolved
//     from the signs on that face alone (the two inside corners are separated), and no triangle edge inside a cube joins
//     two vertices of one face, so the mesh is crack-free and every undirected edge of a closed surface is used by
//     exactly two triangles, in opposite directions;
//   * orientation: (v1 - v0) x (v2 - v0) points towards increasing values: a closed surface encloses the < level region;
//   * vertices: an edge carries one when both ends are finite and on different sides, at t = (level - a) / (b - a) from
//     its lower end a; its normal is the normalised linear interpolation of the central-difference gradients (index units,
//     one-sided at the lattice border) of the two ends (0 when that vanishes);
//   * vertex order, independent of the slab cut: by lattice plane k; inside a plane first the x- and y-edges ordered by
//     (linear index in the plane, axis), then the z-edges from plane k to k + 1.  A slab emits the vertices of its planes
//     0 .. nzs - 1 (and of the x/y edges of plane nzs when it is the last one); the ids of plane nzs's x/y edges follow
//     from that plane alone, so the slab's triangles can name the vertices the next slab emits;
//   * triangles by linear cube index (z slowest), then table order; a cube with a non-finite corner emits nothing;
//   * no atomics: counts per block -> one scan -> emission at the scanned offsets, bit-identical from run to run.
//
// Chain per slab: k_mc_count (per block of 256 lattice points of one plane: x/y-edge vertices, z-edge vertices, triangles,
// reduced with ballot / popcount) -> k_mc_scan (two single-workgroup scans: the vertex counts in vertex order -- plane k:
// all x/y blocks, then all z blocks -- and the triangle counts) -> k_mc_emit_verts (positions, normals, and the global id of
// every edge vertex, vid [3][nzs + 1][ny nx]) -> k_mc_emit_tris (the table staged in LDS, ids from vid).
#define MC_THREADS 256
#define MC_SCAN_THREADS 1024
#define MC_SCAN_PER 4

alignas(16) __device__ const signed char k_mc_tri[256][16] = {
    {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 3, 9, 9, 3, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 10, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 1, 10, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 2, 2, 9, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 3, 10, 10, 3, 9, 9, 3, 8, -1, -1, -1, -1, -1, -1, -1},
    {2, 11, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 2, 8, 8, 2, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 2, 11, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 2, 9, 9, 2, 8, 8, 2, 11, -1, -1, -1, -1, -1, -1, -1},
    {1, 10, 3, 3, 10, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 1, 8, 8, 1, 11, 11, 1, 10, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 3, 3, 9, 11, 11, 9, 10, -1, -1, -1, -1, -1, -1, -1},
    {8, 9, 11, 11, 9, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {4, 8, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 4, 4, 3, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 4, 8, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 3, 9, 9, 3, 4, 4, 3, 7, -1, -1, -1, -1, -1, -1, -1},
    {1, 10, 2, 4, 8, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 4, 4, 3, 7, 1, 10, 2, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 2, 2, 9, 10, 4, 8, 7, -1, -1, -1, -1, -1, -1, -1},
    {2, 3, 10, 10, 3, 9, 9, 3, 4, 4, 3, 7, -1, -1, -1, -1},
    {2, 11, 3, 4, 8, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 2, 4, 4, 2, 7, 7, 2, 11, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 2, 11, 3, 4, 8, 7, -1, -1, -1, -1, -1, -1, -1},
    {1, 2, 9, 9, 2, 4, 4, 2, 7, 7, 2, 11, -1, -1, -1, -1},
    {1, 10, 3, 3, 10, 11, 4, 8, 7, -1, -1, -1, -1, -1, -1, -1},
    {0, 1, 4, 4, 1, 7, 7, 1, 11, 11, 1, 10, -1, -1, -1, -1},
    {0, 9, 3, 3, 9, 11, 11, 9, 10, 4, 8, 7, -1, -1, -1, -1},
    {4, 9, 7, 7, 9, 11, 11, 9, 10, -1, -1, -1, -1, -1, -1, -1},
    {4, 5, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 4, 5, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 4, 1, 1, 4, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 3, 5, 5, 3, 4, 4, 3, 8, -1, -1, -1, -1, -1, -1, -1},
    {1, 10, 2, 4, 5, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 1, 10, 2, 4, 5, 9, -1, -1, -1, -1, -1, -1, -1},
    {0, 4, 2, 2, 4, 10, 10, 4, 5, -1, -1, -1, -1, -1, -1, -1},
    {2, 3, 10, 10, 3, 5, 5, 3, 4, 4, 3, 8, -1, -1, -1, -1},
    {2, 11, 3, 4, 5, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 2, 8, 8, 2, 11, 4, 5, 9, -1, -1, -1, -1, -1, -1, -1},
    {0, 4, 1, 1, 4, 5, 2, 11, 3, -1, -1, -1, -1, -1, -1, -1},
    {1, 2, 5, 5, 2, 4, 4, 2, 8, 8, 2, 11, -1, -1, -1, -1},
    {1, 10, 3, 3, 10, 11, 4, 5, 9, -1, -1, -1, -1, -1, -1, -1},
    {0, 1, 8, 8, 1, 11, 11, 1, 10, 4, 5, 9, -1, -1, -1, -1},
    {0, 4, 3, 3, 4, 11, 11, 4, 10, 10, 4, 5, -1, -1, -1, -1},
    {4, 5, 8, 8, 5, 11, 11, 5, 10, -1, -1, -1, -1, -1, -1, -1},
    {5, 9, 7, 7, 9, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 9, 9, 3, 5, 5, 3, 7, -1, -1, -1, -1, -1, -1, -1},
    {0, 8, 1, 1, 8, 5, 5, 8, 7, -1, -1, -1, -1, -1, -1, -1},
    {1, 3, 5, 5, 3, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 10, 2, 5, 9, 7, 7, 9, 8, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 9, 9, 3, 5, 5, 3, 7, 1, 10, 2, -1, -1, -1, -1},
    {0, 8, 2, 2, 8, 10, 10, 8, 5, 5, 8, 7, -1, -1, -1, -1},
    {2, 3, 10, 10, 3, 5, 5, 3, 7, -1, -1, -1, -1, -1, -1, -1},
    {2, 11, 3, 5, 9, 7, 7, 9, 8, -1, -1, -1, -1, -1, -1, -1},
    {0, 2, 9, 9, 2, 5, 5, 2, 7, 7, 2, 11, -1, -1, -1, -1},
    {0, 8, 1, 1, 8, 5, 5, 8, 7, 2, 11, 3, -1, -1, -1, -1},
    {1, 2, 5, 5, 2, 7, 7, 2, 11, -1, -1, -1, -1, -1, -1, -1},
    {1, 10, 3, 3, 10, 11, 5, 9, 7, 7, 9, 8, -1, -1, -1, -1},
    {0, 7, 9, 9, 7, 5, 0, 1, 7, 7, 1, 11, 11, 1, 10, -1},
    {0, 10, 3, 3, 10, 11, 0, 8, 10, 10, 8, 5, 5, 8, 7, -1},
    {5, 10, 7, 7, 10, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {5, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 5, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 5, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 3, 9, 9, 3, 8, 5, 6, 10, -1, -1, -1, -1, -1, -1, -1},
    {1, 5, 2, 2, 5, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 1, 5, 2, 2, 5, 6, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 2, 2, 9, 6, 6, 9, 5, -1, -1, -1, -1, -1, -1, -1},
    {2, 3, 6, 6, 3, 5, 5, 3, 9, 9, 3, 8, -1, -1, -1, -1},
    {2, 11, 3, 5, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 2, 8, 8, 2, 11, 5, 6, 10, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 2, 11, 3, 5, 6, 10, -1, -1, -1, -1, -1, -1, -1},
    {1, 2, 9, 9, 2, 8, 8, 2, 11, 5, 6, 10, -1, -1, -1, -1},
    {1, 5, 3, 3, 5, 11, 11, 5, 6, -1, -1, -1, -1, -1, -1, -1},
    {0, 1, 8, 8, 1, 11, 11, 1, 6, 6, 1, 5, -1, -1, -1, -1},
    {0, 9, 3, 3, 9, 11, 11, 9, 6, 6, 9, 5, -1, -1, -1, -1},
    {5, 6, 9, 9, 6, 8, 8, 6, 11, -1, -1, -1, -1, -1, -1, -1},
    {4, 8, 7, 5, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 4, 4, 3, 7, 5, 6, 10, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 4, 8, 7, 5, 6, 10, -1, -1, -1, -1, -1, -1, -1},
    {1, 3, 9, 9, 3, 4, 4, 3, 7, 5, 6, 10, -1, -1, -1, -1},
    {1, 5, 2, 2, 5, 6, 4, 8, 7, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 4, 4, 3, 7, 1, 5, 2, 2, 5, 6, -1, -1, -1, -1},
    {0, 9, 2, 2, 9, 6, 6, 9, 5, 4, 8, 7, -1, -1, -1, -1},
    {2, 3, 6, 6, 3, 5, 5, 3, 9, 9, 3, 4, 4, 3, 7, -1},
    {2, 11, 3, 4, 8, 7, 5, 6, 10, -1, -1, -1, -1, -1, -1, -1},
    {0, 2, 4, 4, 2, 7, 7, 2, 11, 5, 6, 10, -1, -1, -1, -1},
    {0, 9, 1, 2, 11, 3, 4, 8, 7, 5, 6, 10, -1, -1, -1, -1},
    {1, 2, 9, 9, 2, 4, 4, 2, 7, 7, 2, 11, 5, 6, 10, -1},
    {1, 5, 3, 3, 5, 11, 11, 5, 6, 4, 8, 7, -1, -1, -1, -1},
    {0, 1, 4, 4, 1, 7, 7, 1, 11, 11, 1, 6, 6, 1, 5, -1},
    {0, 9, 3, 3, 9, 11, 11, 9, 6, 6, 9, 5, 4, 8, 7, -1},
    {4, 9, 7, 7, 9, 11, 11, 9, 6, 6, 9, 5, -1, -1, -1, -1},
    {4, 6, 9, 9, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 4, 6, 9, 9, 6, 10, -1, -1, -1, -1, -1, -1, -1},
    {0, 4, 1, 1, 4, 10, 10, 4, 6, -1, -1, -1, -1, -1, -1, -1},
    {1, 3, 10, 10, 3, 6, 6, 3, 4, 4, 3, 8, -1, -1, -1, -1},
    {1, 9, 2, 2, 9, 6, 6, 9, 4, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 1, 9, 2, 2, 9, 6, 6, 9, 4, -1, -1, -1, -1},
    {0, 4, 2, 2, 4, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 3, 6, 6, 3, 4, 4, 3, 8, -1, -1, -1, -1, -1, -1, -1},
    {2, 11, 3, 4, 6, 9, 9, 6, 10, -1, -1, -1, -1, -1, -1, -1},
    {0, 2, 8, 8, 2, 11, 4, 6, 9, 9, 6, 10, -1, -1, -1, -1},
    {0, 4, 1, 1, 4, 10, 10, 4, 6, 2, 11, 3, -1, -1, -1, -1},
    {1, 4, 10, 10, 4, 6, 1, 2, 4, 4, 2, 8, 8, 2, 11, -1},
    {1, 9, 3, 3, 9, 11, 11, 9, 6, 6, 9, 4, -1, -1, -1, -1},
    {0, 1, 8, 8, 1, 11, 11, 1, 6, 6, 1, 4, 4, 1, 9, -1},
    {0, 4, 3, 3, 4, 11, 11, 4, 6, -1, -1, -1, -1, -1, -1, -1},
    {4, 6, 8, 8, 6, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {6, 10, 7, 7, 10, 8, 8, 10, 9, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 9, 9, 3, 10, 10, 3, 6, 6, 3, 7, -1, -1, -1, -1},
    {0, 8, 1, 1, 8, 10, 10, 8, 6, 6, 8, 7, -1, -1, -1, -1},
    {1, 3, 10, 10, 3, 6, 6, 3, 7, -1, -1, -1, -1, -1, -1, -1},
    {1, 9, 2, 2, 9, 6, 6, 9, 7, 7, 9, 8, -1, -1, -1, -1},
    {0, 3, 9, 9, 6, 1, 1, 6, 2, 9, 3, 6, 6, 3, 7, -1},
    {0, 8, 2, 2, 8, 6, 6, 8, 7, -1, -1, -1, -1, -1, -1, -1},
    {2, 3, 6, 6, 3, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 11, 3, 6, 10, 7, 7, 10, 8, 8, 10, 9, -1, -1, -1, -1},
    {0, 2, 9, 9, 7, 10, 10, 7, 6, 9, 2, 7, 7, 2, 11, -1},
    {0, 8, 1, 1, 8, 10, 10, 8, 6, 6, 8, 7, 2, 11, 3, -1},
    {1, 7, 10, 10, 7, 6, 1, 2, 7, 7, 2, 11, -1, -1, -1, -1},
    {1, 9, 3, 3, 9, 11, 11, 9, 6, 6, 9, 7, 7, 9, 8, -1},
    {0, 1, 9, 6, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 6, 3, 3, 6, 11, 0, 8, 6, 6, 8, 7, -1, -1, -1, -1},
    {6, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {6, 7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 6, 7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 6, 7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 3, 9, 9, 3, 8, 6, 7, 11, -1, -1, -1, -1, -1, -1, -1},
    {1, 10, 2, 6, 7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 1, 10, 2, 6, 7, 11, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 2, 2, 9, 10, 6, 7, 11, -1, -1, -1, -1, -1, -1, -1},
    {2, 3, 10, 10, 3, 9, 9, 3, 8, 6, 7, 11, -1, -1, -1, -1},
    {2, 6, 3, 3, 6, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 2, 8, 8, 2, 7, 7, 2, 6, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 2, 6, 3, 3, 6, 7, -1, -1, -1, -1, -1, -1, -1},
    {1, 2, 9, 9, 2, 8, 8, 2, 7, 7, 2, 6, -1, -1, -1, -1},
    {1, 10, 3, 3, 10, 7, 7, 10, 6, -1, -1, -1, -1, -1, -1, -1},
    {0, 1, 8, 8, 1, 7, 7, 1, 6, 6, 1, 10, -1, -1, -1, -1},
    {0, 9, 3, 3, 9, 7, 7, 9, 6, 6, 9, 10, -1, -1, -1, -1},
    {6, 7, 10, 10, 7, 9, 9, 7, 8, -1, -1, -1, -1, -1, -1, -1},
    {4, 8, 6, 6, 8, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 4, 4, 3, 6, 6, 3, 11, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 4, 8, 6, 6, 8, 11, -1, -1, -1, -1, -1, -1, -1},
    {1, 3, 9, 9, 3, 4, 4, 3, 6, 6, 3, 11, -1, -1, -1, -1},
    {1, 10, 2, 4, 8, 6, 6, 8, 11, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 4, 4, 3, 6, 6, 3, 11, 1, 10, 2, -1, -1, -1, -1},
    {0, 9, 2, 2, 9, 10, 4, 8, 6, 6, 8, 11, -1, -1, -1, -1},
    {2, 3, 10, 10, 3, 9, 9, 3, 4, 4, 3, 6, 6, 3, 11, -1},
    {2, 6, 3, 3, 6, 8, 8, 6, 4, -1, -1, -1, -1, -1, -1, -1},
    {0, 2, 4, 4, 2, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 2, 6, 3, 3, 6, 8, 8, 6, 4, -1, -1, -1, -1},
    {1, 2, 9, 9, 2, 4, 4, 2, 6, -1, -1, -1, -1, -1, -1, -1},
    {1, 10, 3, 3, 10, 8, 8, 10, 4, 4, 10, 6, -1, -1, -1, -1},
    {0, 1, 4, 4, 1, 6, 6, 1, 10, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 3, 3, 6, 8, 8, 6, 4, 3, 9, 6, 6, 9, 10, -1},
    {4, 9, 6, 6, 9, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {4, 5, 9, 6, 7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 4, 5, 9, 6, 7, 11, -1, -1, -1, -1, -1, -1, -1},
    {0, 4, 1, 1, 4, 5, 6, 7, 11, -1, -1, -1, -1, -1, -1, -1},
    {1, 3, 5, 5, 3, 4, 4, 3, 8, 6, 7, 11, -1, -1, -1, -1},
    {1, 10, 2, 4, 5, 9, 6, 7, 11, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 1, 10, 2, 4, 5, 9, 6, 7, 11, -1, -1, -1, -1},
    {0, 4, 2, 2, 4, 10, 10, 4, 5, 6, 7, 11, -1, -1, -1, -1},
    {2, 3, 10, 10, 3, 5, 5, 3, 4, 4, 3, 8, 6, 7, 11, -1},
    {2, 6, 3, 3, 6, 7, 4, 5, 9, -1, -1, -1, -1, -1, -1, -1},
    {0, 2, 8, 8, 2, 7, 7, 2, 6, 4, 5, 9, -1, -1, -1, -1},
    {0, 4, 1, 1, 4, 5, 2, 6, 3, 3, 6, 7, -1, -1, -1, -1},
    {1, 2, 5, 5, 2, 4, 4, 2, 8, 8, 2, 7, 7, 2, 6, -1},
    {1, 10, 3, 3, 10, 7, 7, 10, 6, 4, 5, 9, -1, -1, -1, -1},
    {0, 1, 8, 8, 1, 7, 7, 1, 6, 6, 1, 10, 4, 5, 9, -1},
    {0, 4, 3, 3, 10, 7, 7, 10, 6, 3, 4, 10, 10, 4, 5, -1},
    {4, 5, 8, 8, 10, 7, 7, 10, 6, 8, 5, 10, -1, -1, -1, -1},
    {5, 9, 6, 6, 9, 11, 11, 9, 8, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 9, 9, 3, 5, 5, 3, 6, 6, 3, 11, -1, -1, -1, -1},
    {0, 8, 1, 1, 8, 5, 5, 8, 6, 6, 8, 11, -1, -1, -1, -1},
    {1, 3, 5, 5, 3, 6, 6, 3, 11, -1, -1, -1, -1, -1, -1, -1},
    {1, 10, 2, 5, 9, 6, 6, 9, 11, 11, 9, 8, -1, -1, -1, -1},
    {0, 3, 9, 9, 3, 5, 5, 3, 6, 6, 3, 11, 1, 10, 2, -1},
    {0, 8, 2, 2, 8, 10, 10, 8, 5, 5, 8, 6, 6, 8, 11, -1},
    {2, 3, 10, 10, 3, 5, 5, 3, 6, 6, 3, 11, -1, -1, -1, -1},
    {2, 6, 3, 3, 6, 8, 8, 6, 9, 9, 6, 5, -1, -1, -1, -1},
    {0, 2, 9, 9, 2, 5, 5, 2, 6, -1, -1, -1, -1, -1, -1, -1},
    {0, 8, 1, 1, 8, 5, 5, 8, 6, 6, 8, 2, 2, 8, 3, -1},
    {1, 2, 5, 5, 2, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 10, 3, 3, 10, 8, 8, 6, 9, 9, 6, 5, 8, 10, 6, -1},
    {0, 6, 9, 9, 6, 5, 0, 1, 6, 6, 1, 10, -1, -1, -1, -1},
    {0, 8, 3, 5, 10, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {5, 10, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {5, 7, 10, 10, 7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 5, 7, 10, 10, 7, 11, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 5, 7, 10, 10, 7, 11, -1, -1, -1, -1, -1, -1, -1},
    {1, 3, 9, 9, 3, 8, 5, 7, 10, 10, 7, 11, -1, -1, -1, -1},
    {1, 5, 2, 2, 5, 11, 11, 5, 7, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 1, 5, 2, 2, 5, 11, 11, 5, 7, -1, -1, -1, -1},
    {0, 9, 2, 2, 9, 11, 11, 9, 7, 7, 9, 5, -1, -1, -1, -1},
    {2, 5, 11, 11, 5, 7, 2, 3, 5, 5, 3, 9, 9, 3, 8, -1},
    {2, 10, 3, 3, 10, 7, 7, 10, 5, -1, -1, -1, -1, -1, -1, -1},
    {0, 2, 8, 8, 2, 7, 7, 2, 5, 5, 2, 10, -1, -1, -1, -1},
    {0, 9, 1, 2, 10, 3, 3, 10, 7, 7, 10, 5, -1, -1, -1, -1},
    {1, 2, 9, 9, 2, 8, 8, 2, 7, 7, 2, 5, 5, 2, 10, -1},
    {1, 5, 3, 3, 5, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 1, 8, 8, 1, 7, 7, 1, 5, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 3, 3, 9, 7, 7, 9, 5, -1, -1, -1, -1, -1, -1, -1},
    {5, 7, 9, 9, 7, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {4, 8, 5, 5, 8, 10, 10, 8, 11, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 4, 4, 3, 5, 5, 3, 10, 10, 3, 11, -1, -1, -1, -1},
    {0, 9, 1, 4, 8, 5, 5, 8, 10, 10, 8, 11, -1, -1, -1, -1},
    {1, 3, 9, 9, 3, 4, 4, 3, 5, 5, 3, 10, 10, 3, 11, -1},
    {1, 5, 2, 2, 5, 11, 11, 5, 8, 8, 5, 4, -1, -1, -1, -1},
    {0, 3, 4, 4, 3, 5, 5, 11, 1, 1, 11, 2, 5, 3, 11, -1},
    {0, 9, 2, 2, 9, 11, 11, 5, 8, 8, 5, 4, 11, 9, 5, -1},
    {2, 3, 11, 4, 9, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 10, 3, 3, 10, 8, 8, 10, 4, 4, 10, 5, -1, -1, -1, -1},
    {0, 2, 4, 4, 2, 5, 5, 2, 10, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 1, 2, 10, 3, 3, 10, 8, 8, 10, 4, 4, 10, 5, -1},
    {1, 2, 9, 9, 2, 4, 4, 2, 5, 5, 2, 10, -1, -1, -1, -1},
    {1, 5, 3, 3, 5, 8, 8, 5, 4, -1, -1, -1, -1, -1, -1, -1},
    {0, 1, 4, 4, 1, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 3, 3, 5, 8, 8, 5, 4, 3, 9, 5, -1, -1, -1, -1},
    {4, 9, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {4, 7, 9, 9, 7, 10, 10, 7, 11, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, 4, 7, 9, 9, 7, 10, 10, 7, 11, -1, -1, -1, -1},
    {0, 4, 1, 1, 4, 10, 10, 4, 11, 11, 4, 7, -1, -1, -1, -1},
    {1, 3, 10, 10, 4, 11, 11, 4, 7, 10, 3, 4, 4, 3, 8, -1},
    {1, 9, 2, 2, 9, 11, 11, 9, 7, 7, 9, 4, -1, -1, -1, -1},
    {0, 3, 8, 1, 9, 2, 2, 9, 11, 11, 9, 7, 7, 9, 4, -1},
    {0, 4, 2, 2, 4, 11, 11, 4, 7, -1, -1, -1, -1, -1, -1, -1},
    {2, 4, 11, 11, 4, 7, 2, 3, 4, 4, 3, 8, -1, -1, -1, -1},
    {2, 10, 3, 3, 10, 7, 7, 10, 4, 4, 10, 9, -1, -1, -1, -1},
    {0, 2, 8, 8, 2, 7, 7, 2, 4, 4, 2, 9, 9, 2, 10, -1},
    {0, 4, 1, 1, 4, 10, 10, 4, 2, 2, 4, 3, 3, 4, 7, -1},
    {1, 2, 10, 4, 7, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 9, 3, 3, 9, 7, 7, 9, 4, -1, -1, -1, -1, -1, -1, -1},
    {0, 1, 8, 8, 1, 7, 7, 1, 4, 4, 1, 9, -1, -1, -1, -1},
    {0, 4, 3, 3, 4, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {4, 7, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {8, 11, 9, 9, 11, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 9, 9, 3, 10, 10, 3, 11, -1, -1, -1, -1, -1, -1, -1},
    {0, 8, 1, 1, 8, 10, 10, 8, 11, -1, -1, -1, -1, -1, -1, -1},
    {1, 3, 10, 10, 3, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 9, 2, 2, 9, 11, 11, 9, 8, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 9, 9, 11, 1, 1, 11, 2, 9, 3, 11, -1, -1, -1, -1},
    {0, 8, 2, 2, 8, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 3, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 10, 3, 3, 10, 8, 8, 10, 9, -1, -1, -1, -1, -1, -1, -1},
    {0, 2, 9, 9, 2, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 8, 1, 1, 8, 10, 10, 8, 2, 2, 8, 3, -1, -1, -1, -1},
    {1, 2, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 9, 3, 3, 9, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 1, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 8, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
};
// owner of cube edge e, 5 bits each: di | dj << 1 | dk << 2 | axis << 3
__device__ __forceinline__ int mc_owner_code(int e) {
  // e:      0  1  2  3  4   5  6   7   8   9  10  11
  // code:   0  9  2  8  4  13  6  12  16  17  19  18
  const uint64_t packed = 0ull | (9ull << 5) | (2ull << 10) | (8ull << 15) | (4ull << 20) | (13ull << 25) | (6ull << 30) |
                          (12ull << 35) | (16ull << 40) | (17ull << 45) | (19ull << 50) | (18ull << 55);
  return (int)((packed >> (5 * e)) & 31ull);
}

struct McSlab {
  const float* lat;      // [nzs + 1][ny][nx]
  const float* below;    // plane k = -1 (may be NULL)
  const float* above;    // plane k = nzs + 1 (may be NULL)
  int nx, ny, nzs, bpp;  // bpp: blocks per plane
  int64_t P;             // nx * ny
  float level;
};

__device__ __forceinline__ float mc_at(const McSlab& s, int i, int j, int k) {
  const int64_t q = (int64_t)j * s.nx + i;
  if (k < 0) return s.below[q];
  if (k > s.nzs) return s.above[q];
  return s.lat[(int64_t)k * s.P + q];
}

__device__ __forceinline__ bool mc_cross(float a, float b, float level) {
  return isfinite(a) && isfinite(b) && ((a < level) != (b < level));
}

// case of the cube with origin (i, j, k), -1 if a corner is not finite
__device__ __forceinline__ int mc_case(const McSlab& s, int i, int j, int k) {
  int c = 0;
  bool ok = true;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float v = mc_at(s, i + ((q ^ (q >> 1)) & 1), j + ((q >> 1) & 1), k + (q >> 2));
    ok = ok && isfinite(v);
    c |= (v < s.level ? 1 : 0) << q;
  }
  return ok ? c : -1;
}

// small per-lane counts (0..7) of a wave: ballots of the three bits -> exclusive prefix over the lanes below and total
__device__ __forceinline__ int mc_wave_scan(int c, int& total) {
  const unsigned long long b0 = wave_ballot(c & 1), b1 = wave_ballot(c & 2), b2 = wave_ballot(c & 4);
  const unsigned long long lt = (1ull << nsim_lane()) - 1ull;
  total = __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2);
  return __popcll(b0 & lt) + 2 * __popcll(b1 & lt) + 4 * __popcll(b2 & lt);
}

// the same over the block: exclusive prefix of c among the block's threads, and the block total (NV values at once)
template <int NV>
__device__ __forceinline__ void mc_block_scan(const int (&c)[NV], int (&pre)[NV], int (&tot)[NV], int (*wsum)[NV]) {
  const int wave = threadIdx.x >> 6;
  int wt[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) pre[v] = mc_wave_scan(c[v], wt[v]);
  if (nsim_lane() == 0)
#pragma unroll
    for (int v = 0; v < NV; ++v) wsum[wave][v] = wt[v];
  __syncthreads();
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < MC_THREADS / 64; ++w) {
      before += w < wave ? wsum[w][v] : 0;
      all += wsum[w][v];
    }
    pre[v] += before;
    tot[v] = all;
  }
}

// edge crossings a lattice point owns: x, y (in its plane), z (to the next plane; k < nzs)
__device__ __forceinline__ void mc_point_edges(const McSlab& s, int i, int j, int k, int& cx, int& cy, int& cz) {
  const float f0 = mc_at(s, i, j, k);
  cx = (i + 1 < s.nx && mc_cross(f0, mc_at(s, i + 1, j, k), s.level)) ? 1 : 0;
  cy = (j + 1 < s.ny && mc_cross(f0, mc_at(s, i, j + 1, k), s.level)) ? 1 : 0;
  cz = (k < s.nzs && mc_cross(f0, mc_at(s, i, j, k + 1), s.level)) ? 1 : 0;
}

__global__ void __launch_bounds__(MC_THREADS) k_mc_count(McSlab s, int32_t* __restrict__ cnt_v, int32_t* __restrict__ cnt_t) {
  __shared__ int ntri[256];
  __shared__ int wsum[MC_THREADS / 64][3];
  const int tid = threadIdx.x, k = blockIdx.y, b = blockIdx.x;
  {
    int n = 0;
#pragma unroll
    for (int q = 0; q < 15; q += 3) n += k_mc_tri[tid][q] >= 0 ? 1 : 0;
    ntri[tid] = n;
  }
  __syncthreads();
  const int64_t p = (int64_t)b * MC_THREADS + tid;
  int c[3] = {0, 0, 0};
  if (p < s.P) {
    const int i = (int)(p % s.nx), j = (int)(p / s.nx);
    int cx, cy, cz;
    mc_point_edges(s, i, j, k, cx, cy, cz);
    c[0] = cx + cy;
    c[1] = cz;
    if (k < s.nzs && i + 1 < s.nx && j + 1 < s.ny) {
      const int cs = mc_case(s, i, j, k);
      c[2] = cs >= 0 ? ntri[cs] : 0;
    }
  }
  int pre[3], tot[3];
  mc_block_scan<3>(c, pre, tot, wsum);
  if (tid == 0) {
    cnt_v[((int64_t)k * 2 + 0) * s.bpp + b] = tot[0];
    cnt_v[((int64_t)k * 2 + 1) * s.bpp + b] = tot[1];
    cnt_t[(int64_t)k * s.bpp + b] = tot[2];
  }
}

// block 0: exclusive scan of the vertex counts in place (n_v entries; tot[0] = the value at split_v, tot[1] = the total);
// block 1: of the triangle counts (tot[2] = the total)
__global__ void __launch_bounds__(MC_SCAN_THREADS) k_mc_scan(int32_t* __restrict__ cnt_v, int64_t n_v, int64_t split_v,
                                                           int32_t* __restrict__ cnt_t, int64_t n_t, int32_t* __restrict__ tot) {
  __shared__ int wtot[MC_SCAN_THREADS / 64];
  const int tid = threadIdx.x, lane = nsim_lane(), wave = tid >> 6;
  int32_t* a = blockIdx.x == 0 ? cnt_v : cnt_t;
  const int64_t n = blockIdx.x == 0 ? n_v : n_t;
  int carry = 0;
  for (int64_t base = 0; base < n; base += (int64_t)MC_SCAN_THREADS * MC_SCAN_PER) {
    const int64_t i0 = base + (int64_t)tid * MC_SCAN_PER;
    int v[MC_SCAN_PER];
    int mine = 0;
#pragma unroll
    for (int q = 0; q < MC_SCAN_PER; ++q) {
      v[q] = (i0 + q) < n ? a[i0 + q] : 0;
      mine += v[q];
    }
    const int incl = wave_incl_sum(mine);
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int before = 0, chunk = 0;
#pragma unroll
    for (int w = 0; w < MC_SCAN_THREADS / 64; ++w) {
      const int x = wtot[w];
      before += (w < wave) ? x : 0;
      chunk += x;
    }
    int run = carry + before + incl - mine;
#pragma unroll
    for (int q = 0; q < MC_SCAN_PER; ++q) {
      const int64_t i = i0 + q;
      if (i < n) {
        a[i] = run;
        if (blockIdx.x == 0 && i == split_v) tot[0] = run;
      }
      run += v[q];
    }
    carry += chunk;
    __syncthreads();
  }
  if (tid == 0) {
    if (blockIdx.x == 0) {
      tot[1] = carry;
      if (split_v >= n) tot[0] = carry;
    } else {
      tot[2] = carry;
    }
  }
}

// central difference in index units along one axis (one-sided where a neighbour is missing)
__device__ __forceinline__ float mc_diff(float fm, float f0, float fp, bool hm, bool hp) {
  return (hm && hp) ? (fp - fm) * 0.5f : hp ? (fp - f0) : hm ? (f0 - fm) : 0.f;
}

__device__ __forceinline__ void mc_grad(const McSlab& s, int i, int j, int k, float g[3]) {
  const float f0 = mc_at(s, i, j, k);
  const bool xm = i > 0, xp = i + 1 < s.nx, ym = j > 0, yp = j + 1 < s.ny;
  const bool zm = k > 0 || s.below != nullptr, zp = k < s.nzs || s.above != nullptr;
  g[0] = mc_diff(xm ? mc_at(s, i - 1, j, k) : 0.f, f0, xp ? mc_at(s, i + 1, j, k) : 0.f, xm, xp);
  g[1] = mc_diff(ym ? mc_at(s, i, j - 1, k) : 0.f, f0, yp ? mc_at(s, i, j + 1, k) : 0.f, ym, yp);
  g[2] = mc_diff(zm ? mc_at(s, i, j, k - 1) : 0.f, f0, zp ? mc_at(s, i, j, k + 1) : 0.f, zm, zp);
}

struct McPlace {
  float bx, by, bz, h;
  int64_t k0;    // global index of the slab's plane 0
  int64_t vbase; // global id of the slab's first vertex
};

__device__ __forceinline__ void mc_vertex(const McSlab& s, const McPlace& pl, int i, int j, int k, int ax, float* __restrict__ verts,
                                          float* __restrict__ normals, int64_t o) {
  const int di = ax == 0, dj = ax == 1, dk = ax == 2;
  const float a = mc_at(s, i, j, k), b = mc_at(s, i + di, j + dj, k + dk);
  const float t = (s.level - a) / (b - a);
  float fi[3] = {(float)i, (float)j, (float)(pl.k0 + k)};
  fi[ax] = fi[ax] + t;
  verts[3 * o + 0] = pl.bx + pl.h * fi[0];
  verts[3 * o + 1] = pl.by + pl.h * fi[1];
  verts[3 * o + 2] = pl.bz + pl.h * fi[2];
  float ga[3], gb[3], n[3];
  mc_grad(s, i, j, k, ga);
  mc_grad(s, i + di, j + dj, k + dk, gb);
#pragma unroll
  for (int q = 0; q < 3; ++q) n[q] = (1.f - t) * ga[q] + t * gb[q];
  const float ln = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  const bool ok = ln > 0.f && isfinite(ln);
#pragma unroll
  for (int q = 0; q < 3; ++q) normals[3 * o + q] = ok ? n[q] / ln : 0.f;
}

__global__ void __launch_bounds__(MC_THREADS) k_mc_emit_verts(McSlab s, McPlace pl, int emit_top, const int32_t* __restrict__ off_v,
                                                            int32_t* __restrict__ vid, float* __restrict__ verts,
                                                            float* __restrict__ normals) {
  __shared__ int wsum[MC_THREADS / 64][2];
  const int tid = threadIdx.x, k = blockIdx.y, b = blockIdx.x;
  const int64_t p = (int64_t)b * MC_THREADS + tid;
  int cx = 0, cy = 0, cz = 0, i = 0, j = 0;
  if (p < s.P) {
    i = (int)(p % s.nx);
    j = (int)(p / s.nx);
    mc_point_edges(s, i, j, k, cx, cy, cz);
  }
  const int c[2] = {cx + cy, cz};
  int pre[2], tot[2];
  mc_block_scan<2>(c, pre, tot, wsum);
  if (p >= s.P) return;
  const int64_t oxy = (int64_t)off_v[((int64_t)k * 2 + 0) * s.bpp + b] + pre[0];
  const int64_t oz = (int64_t)off_v[((int64_t)k * 2 + 1) * s.bpp + b] + pre[1];
  const int64_t N = (int64_t)(s.nzs + 1) * s.P, q = (int64_t)k * s.P + p;
  vid[q] = cx ? (int32_t)(pl.vbase + oxy) : -1;
  vid[N + q] = cy ? (int32_t)(pl.vbase + oxy + cx) : -1;
  vid[2 * N + q] = cz ? (int32_t)(pl.vbase + oz) : -1;
  if (k == s.nzs && !emit_top) return;
  if (cx) mc_vertex(s, pl, i, j, k, 0, verts, normals, oxy);
  if (cy) mc_vertex(s, pl, i, j, k, 1, verts, normals, oxy + cx);
  if (cz) mc_vertex(s, pl, i, j, k, 2, verts, normals, oz);
}

__global__ void __launch_bounds__(MC_THREADS) k_mc_emit_tris(McSlab s, const int32_t* __restrict__ off_t,
                                                           const int32_t* __restrict__ vid, int32_t* __restrict__ faces) {
  __shared__ __attribute__((aligned(16))) signed char tab[256 * 16];
  __shared__ int ntri[256];
  __shared__ int wsum[MC_THREADS / 64][1];
  const int tid = threadIdx.x, k = blockIdx.y, b = blockIdx.x;
  {   // stage the table: one 16-byte row per thread (256 x 16 int8 = 4 KB)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      reinterpret_cast<uint32_t*>(tab)[4 * tid + q] = reinterpret_cast<const uint32_t*>(&k_mc_tri[0][0])[4 * tid + q];
    int n = 0;
#pragma unroll
    for (int q = 0; q < 15; q += 3) n += k_mc_tri[tid][q] >= 0 ? 1 : 0;
    ntri[tid] = n;
  }
  __syncthreads();
  const int64_t p = (int64_t)b * MC_THREADS + tid;
  int cs = -1, i = 0, j = 0;
  if (p < s.P) {
    i = (int)(p % s.nx);
    j = (int)(p / s.nx);
    if (i + 1 < s.nx && j + 1 < s.ny) cs = mc_case(s, i, j, k);
  }
  const int c[1] = {cs >= 0 ? ntri[cs] : 0};
  int pre[1], tot[1];
  mc_block_scan<1>(c, pre, tot, wsum);
  if (c[0] == 0) return;
  const int64_t o = (int64_t)off_t[(int64_t)k * s.bpp + b] + pre[0];
  const int64_t N = (int64_t)(s.nzs + 1) * s.P;
  for (int q = 0; q < 3 * c[0]; ++q) {
    const int code = mc_owner_code(tab[cs * 16 + q]);
    const int di = code & 1, dj = (code >> 1) & 1, dk = (code >> 2) & 1, ax = code >> 3;
    faces[3 * o + q] = vid[ax * N + (int64_t)(k + dk) * s.P + (int64_t)(j + dj) * s.nx + (i + di)];
  }
}

static int mc_slab(const float* lat, const float* below, const float* above, int64_t nx, int64_t ny, int64_t nzs, float level,
                   McSlab& s) {
  if (nx < 1 || ny < 1 || nzs < 0) return 2;
  if (nzs + 1 > 65535 || nx * ny >= ((int64_t)1 << 31) || nx >= ((int64_t)1 << 30)) return 50;
  if (!lat) return 4;
  s.lat = lat;
  s.below = below;
  s.above = above;
  s.nx = (int)nx;
  s.ny = (int)ny;
  s.nzs = (int)nzs;
  s.P = nx * ny;
  s.bpp = (int)((s.P + MC_THREADS - 1) / MC_THREADS);
  s.level = level;
  return 0;
}

extern "C" {

int nsim_mc_count(const float* lat, int64_t nx, int64_t ny, int64_t nzs, float level, int32_t* cnt_v, int32_t* cnt_t,
                  void* stream) {
  McSlab s;
  const int rc = mc_slab(lat, nullptr, nullptr, nx, ny, nzs, level, s);
  if (rc) return rc;
  if (!cnt_v || !cnt_t) return 4;
  hipLaunchKernelGGL(k_mc_count, dim3(s.bpp, s.nzs + 1), dim3(MC_THREADS), 0, (hipStream_t)stream, s, cnt_v, cnt_t);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_mc_scan(int32_t* cnt_v, int32_t* cnt_t, int64_t nx, int64_t ny, int64_t nzs, int32_t* totals, void* stream) {
  if (nx < 1 || ny < 1 || nzs < 0) return 2;
  if (!cnt_v || !cnt_t || !totals) return 4;
  const int64_t bpp = (nx * ny + MC_THREADS - 1) / MC_THREADS, nv = (nzs + 1) * 2 * bpp, nt = (nzs + 1) * bpp;
  hipLaunchKernelGGL(k_mc_scan, dim3(2), dim3(MC_SCAN_THREADS), 0, (hipStream_t)stream, cnt_v, nv, nzs * 2 * bpp, cnt_t, nt,
                     totals);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_mc_emit_verts(const float* lat, const float* below, const float* above, int64_t nx, int64_t ny, int64_t nzs, float level,
                       float bx, float by, float bz, float h, int64_t k0, int64_t vbase, int emit_top, const int32_t* off_v,
                       int32_t* vid, float* verts, float* normals, void* stream) {
  McSlab s;
  const int rc = mc_slab(lat, below, above, nx, ny, nzs, level, s);
  if (rc) return rc;
  if (!off_v || !vid || !verts || !normals) return 4;
  McPlace pl;
  pl.bx = bx;
  pl.by = by;
  pl.bz = bz;
  pl.h = h;
  pl.k0 = k0;
  pl.vbase = vbase;
  hipLaunchKernelGGL(k_mc_emit_verts, dim3(s.bpp, s.nzs + 1), dim3(MC_THREADS), 0, (hipStream_t)stream, s, pl, emit_top, off_v, vid,
                     verts, normals);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_mc_emit_tris(const float* lat, int64_t nx, int64_t ny, int64_t nzs, float level, const int32_t* off_t, const int32_t* vid,
                      int32_t* faces, void* stream) {
  McSlab s;
  const int rc = mc_slab(lat, nullptr, nullptr, nx, ny, nzs, level, s);
  if (rc) return rc;
  if (nzs == 0) return 0;
  if (!off_t || !vid || !faces) return 4;
  hipLaunchKernelGGL(k_mc_emit_tris, dim3(s.bpp, s.nzs), dim3(MC_THREADS), 0, (hipStream_t)stream, s, off_t, vid, faces);
  NSIM_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

extern "C" {

int nsim_version(void) { return 100; }

const char* nsim_strerror(int code) {
  switch (code) {
    case 0: return "ok";
    case 2: return "negative size";
    case 3: return "bad channel count / op code";
    case 4: return "required output pointer is NULL";
    case 5: return "missing occupancy/AABB meta or non-positive step";
    case 10: return "LoTD meta is NULL";
    case 11: return "LoTD n_feats must be 2";
    case 12: return "LoTD num_levels out of range";
    case 13: return "LoTD level resolution < 2";
    case 14: return "LoTD dense level size != res^3";
    case 15: return "LoTD unknown level type";
    case 16: return "LoTD level offset must be even";
    case 17: return "LoTD hash table size must be a power of two";
    case 29: return "per-ray instance offsets (batched model) need ridx";
    case 28: return "h / dh/dx planes (and dh / g hand-off planes when dgrid is requested) are required";
    case 27: return "radiance backward needs the saved forward nablas / rgb and a [S,3] scratch buffer";
    case 30: return "sky meta is NULL";
    case 31: return "sky input width 3 + 6 n_frequencies + n_appear must be <= 96";
    case 32: return "sky model with n_appear > 0 needs h_appear";
    case 20: return "field meta is NULL";
    case 21: return "field kernels take 1..32 LoTD levels (<= 64 input features)";
    case 33: return "pyramids with more than 16 levels exist on the level-major path only: the planes arguments are required";
    case 40: return "permuto meta is NULL";
    case 41: return "permuto in_dim must be 2..8 (>= 3 for the field front end)";
    case 42: return "permuto num_levels must be 1..32";
    case 43: return "permuto n_feats must be 2";
    case 44: return "permuto hashmap_size must be a power of two";
    case 34: return "too many (device, stream) pairs with a registered gradient scratch (64)";
    case 22: return "sdf_D must be 1 or 2";
    case 23: return "precision must be 0 (fp16 MFMA) or 1 (f32 MFMA)";
    case 24: return "need either x or (rays_o, rays_d, t, ridx)";
    case 25: return "radiance needs rays_d and ridx";
    case 26: return "gradient output pointer is NULL";
    case 37: return "compose collect: at most 64 sources";
    case 50: return "marching cubes: lattice sizes out of range (nx * ny < 2^31, at most 65534 cubes per slab in z)";
    case 36: return "wide decoder: 0..10 embedding frequencies and at most 128 first-layer inputs (2 num_levels + 3 + 6 n_freq)";
    default: return code >= 1000 ? "HIP launch error (code - 1000 = hipError_t)" : "unknown error";
  }
}

}  // extern "C"
