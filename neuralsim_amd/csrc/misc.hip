// misc.hip -- version / error strings of the C ABI, marching cubes on slabs of SDF lattices (nsim_mc_*), and exact nearest-neighbour
// search between point clouds (nsim_nn_*), occupancy grids from lattices of SDF values (nsim_occgrid_*), and visible grids
// from rendered samples (nsim_vgrid_*).
#include "nsim_common.h"
#include "occ_dev.h"

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

// exclusive scan of a[0 .. n) in place by one workgroup of MC_SCAN_THREADS threads -> the total (in every thread); the scanned
// value at index split (if 0 <= split < n) is also written to *at_split.  Shared by k_mc_scan and k_nn_scan.
__device__ __forceinline__ int block_excl_scan_inplace(int32_t* __restrict__ a, int64_t n, int64_t split, int32_t* at_split,
                                                       int* wtot) {
  const int tid = threadIdx.x, lane = nsim_lane(), wave = tid >> 6;
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
        if (i == split) *at_split = run;
      }
      run += v[q];
    }
    carry += chunk;
    __syncthreads();
  }
  return carry;
}

// block 0: exclusive scan of the vertex counts in place (n_v entries; tot[0] = the value at split_v, tot[1] = the total);
// block 1: of the triangle counts (tot[2] = the total)
__global__ void __launch_bounds__(MC_SCAN_THREADS) k_mc_scan(int32_t* __restrict__ cnt_v, int64_t n_v, int64_t split_v,
                                                           int32_t* __restrict__ cnt_t, int64_t n_t, int32_t* __restrict__ tot) {
  __shared__ int wtot[MC_SCAN_THREADS / 64];
  if (blockIdx.x == 0) {
    const int carry = block_excl_scan_inplace(cnt_v, n_v, split_v, &tot[0], wtot);
    if (threadIdx.x == 0) {
      tot[1] = carry;
      if (split_v >= n_v) tot[0] = carry;
    }
  } else {
    const int carry = block_excl_scan_inplace(cnt_t, n_t, -1, nullptr, wtot);
    if (threadIdx.x == 0) tot[2] = carry;
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

// ------------------------------------------------------------------------------------------------ nearest neighbours
// nr3d_lib.maths.chamfer_distance (code_single/tools/eval_lidar.py:417-421), the kernels behind neuralsim_amd/pointcloud.py.
//
// For every query x[i]: d2[i] = min_j nn_dist2(x[i], y[j]) in f32 and idx[i] = the LOWEST j that attains it.  Points of y with a
// non-finite coordinate are never selected (their distance is inf or NaN, and a candidate replaces the running best only when
// it compares strictly lower, or equal with a lower index); a query nothing was selected for (non-finite query, empty y, or
// every distance overflowing) gets d2 = +inf, idx = -1.  Every path goes through nn_dist2 and the same tie rule, so the result
// is a function of the inputs alone: not of the path, of the order in which points were binned, or of the run.
//
// Path a, k_nn_brute: one thread per query, y streamed through LDS in structure-of-arrays tiles of NN_TILE points read as
// wave-wide broadcasts of 4 points per ds_read_b128.  With nsplit > 1 workgroup (bx, by) searches y's chunk by for the
// queries of bx and writes a partial (d2, idx); k_nn_combine takes the minimum of the partials in chunk order (chunks ascend
// in j, so a strict < keeps the lowest index).  With a query list the kernel reads the list's length from device memory and
// at most NN_LIST_BLOCKS query blocks are launched and stride over it: the leftovers of path b are finished without the host knowing how many there are.
//
// Path b, uniform grid over the bounding box of y's finite points, everything on the device:
//   k_nn_bbox (bounding box and count of the finite points; order-preserving integer encoding of the floats, integer atomic
//   min) -> k_nn_grid_setup (one thread: cubic cell size and resolution, NnGrid below) -> k_nn_grid_count (cell of every
//   point; rank inside its cell = the return value of the integer atomic increment of the cell's count) -> k_nn_scan
//   (exclusive offsets of the cells, x fastest) -> k_nn_grid_fill (records (x, y, z, original index) at offset + rank) ->
//   k_nn_grid_query.  A point's rank inside its cell depends on the arrival order of the atomics, the results do not: ties
//   are broken on the original index carried in the record.
//
// Cell size: the clouds this is for (LiDAR sweeps, mesh vertices) are surfaces, so a box of n points holds about
// n h^2 / (e1 e2) points per occupied cell of side h, e1 >= e2 the box's two largest extents:
// h = sqrt(target_occ e1 e2 / n); from the box VOLUME it would come out far too coarse for a flat cloud (a line: h =
// target_occ e1 / n).  h then grows by 1.25 until the cell count fits max_cells (the caller's workspace).
#define NN_THREADS 256
#define NN_TILE 1024
#define NN_HDR_INTS 32
#define NN_COARSE_FACTOR 16.f
#define NN_LIST_BLOCKS 1024   // at most this many query blocks are launched for a device-side query list (the kernel strides over it)

typedef float nn_f4 __attribute__((ext_vector_type(4)));

// one point of y in cell order: 16 bytes, read whole
struct alignas(16) NnRec {
  float x, y, z;
  int32_t j;   // index in y
};

// the one distance of every path: f32, (dx dx + dy dy) + dz dz, no contraction (the library is built with -ffp-contract=off)
__device__ __forceinline__ float nn_dist2(float qx, float qy, float qz, float px, float py, float pz) {
  const float dx = qx - px, dy = qy - py, dz = qz - pz;
  return (dx * dx + dy * dy) + dz * dz;
}

// does candidate (d, j) replace (best, bi)?  false for NaN / inf against the initial (inf, -1)
__device__ __forceinline__ bool nn_better(float d, int j, float best, int bi) { return d < best || (d == best && j < bi); }

__device__ __forceinline__ bool nn_finite3(float a, float b, float c) { return isfinite(a) && isfinite(b) && isfinite(c); }

// header of the grid workspace (int32 / f32 [NN_HDR_INTS]): written on the device, read by every kernel of path b
struct NnGrid {
  uint32_t box[6];   // encoded min x, y, z and complement of the encoded max x, y, z of the finite points (atomic min)
  int32_t n_finite;  // finite points of y
  int32_t n_left;    // queries handed to the exhaustive pass
  int32_t res[3];    // cells per axis
  int32_t ncells;
  float bmin[3];
  float h, inv_h;    // cell side, and the f32 reciprocal every cell coordinate is formed with
  int32_t n_occ;     // cells that hold at least one point
  float target_occ;  // the occupancy the cell size aimed at
  int32_t pad[13];
};
static_assert(sizeof(NnGrid) == 4 * NN_HDR_INTS, "NnGrid is the header of the grid workspace");

// order-preserving map of finite floats to uint32
__device__ __forceinline__ uint32_t nn_enc(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float nn_dec(uint32_t e) {
  const uint32_t u = (e & 0x80000000u) ? (e & 0x7fffffffu) : ~e;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// cell coordinate of p along one axis, in cells, as a float.  Monotone in p (a rounded subtraction and a rounded product with a
// positive constant are monotone); the cell index is its floor clamped to [0, res - 1].  The points of y and the queries go
// through this one function: the stopping rule of k_nn_grid_query rests on that.
__device__ __forceinline__ float nn_cell_coord(float p, float bmin, float inv_h) { return (p - bmin) * inv_h; }
__device__ __forceinline__ int nn_cell_index(float u, int res) { return (int)fminf(fmaxf(u, 0.f), (float)(res - 1)); }

__global__ void __launch_bounds__(NN_THREADS) k_nn_bbox(const float* __restrict__ y, int64_t M, NnGrid* __restrict__ g) {
  __shared__ uint32_t sm[NN_THREADS / 64][6];
  __shared__ int sn[NN_THREADS / 64];
  uint32_t e[6] = {~0u, ~0u, ~0u, ~0u, ~0u, ~0u};
  int n = 0;
  for (int64_t j = (int64_t)blockIdx.x * NN_THREADS + threadIdx.x; j < M; j += (int64_t)gridDim.x * NN_THREADS) {
    const float p[3] = {y[3 * j], y[3 * j + 1], y[3 * j + 2]};
    if (!nn_finite3(p[0], p[1], p[2])) continue;
    ++n;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const uint32_t c = nn_enc(p[a]);
      e[a] = c < e[a] ? c : e[a];
      e[3 + a] = ~c < e[3 + a] ? ~c : e[3 + a];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const uint32_t u = wave_shfl_xor(e[a], o);
      e[a] = u < e[a] ? u : e[a];
    }
  }
  n = wave_sum(n);
  const int wave = threadIdx.x >> 6;
  if (nsim_lane() == 0) {
#pragma unroll
    for (int a = 0; a < 6; ++a) sm[wave][a] = e[a];
    sn[wave] = n;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    uint32_t m = sm[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < NN_THREADS / 64; ++w) m = sm[w][threadIdx.x] < m ? sm[w][threadIdx.x] : m;
    atomicMin(&g->box[threadIdx.x], m);
  } else if (threadIdx.x == 6) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < NN_THREADS / 64; ++w) t += sn[w];
    if (t) atomicAdd(&g->n_finite, t);
  }
}

__global__ void __launch_bounds__(64) k_nn_grid_setup(NnGrid* __restrict__ g, float target_occ, int64_t max_cells) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int n = g->n_finite;
  float bmin[3] = {0.f, 0.f, 0.f}, e[3] = {0.f, 0.f, 0.f};
  if (n > 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      bmin[a] = nn_dec(g->box[a]);
      e[a] = nn_dec(~g->box[3 + a]) - bmin[a];
    }
  }
  // the two largest extents
  const float emax = fmaxf(e[0], fmaxf(e[1], e[2])), emin = fminf(e[0], fminf(e[1], e[2]));
  const float emid = (e[0] + e[1] + e[2]) - emax - emin;
  float h = 0.f;
  if (n > 0 && isfinite(e[0] + e[1] + e[2])) {
    if (emid > 0.f && emid >= emax * 1e-6f) h = sqrtf(target_occ * (emax / (float)n) * emid);
    else h = target_occ * emax / (float)n;
    h = fmaxf(h, emax * (1.f / 1048576.f));   // at most 2^20 cells per axis: cell indices are exact in f32
  }
  int res[3] = {1, 1, 1};
  float inv_h = 1.f;
  if (h > 0.f && isfinite(h) && isfinite(1.f / h)) {
    for (int it = 0; it < 256; ++it) {
      inv_h = 1.f / h;
      int64_t total = 1;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        res[a] = (int)fminf(e[a] * inv_h, 1048575.f) + 1;
        total *= res[a];
      }
      if (total <= max_cells) break;
      h *= 1.25f;
    }
  } else {
    h = 1.f;   // no finite point, a single point, or extents that overflow: one cell
  }
  if ((int64_t)res[0] * res[1] * res[2] > max_cells || !(inv_h > 0.f) || !isfinite(inv_h)) {
    res[0] = res[1] = res[2] = 1;
    h = inv_h = 1.f;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    g->res[a] = res[a];
    g->bmin[a] = bmin[a];
  }
  g->ncells = res[0] * res[1] * res[2];
  g->h = h;
  g->inv_h = inv_h;
  g->target_occ = target_occ;
}

__global__ void __launch_bounds__(NN_THREADS) k_nn_grid_count(const float* __restrict__ y, int64_t M, NnGrid* __restrict__ g,
                                                            int32_t* __restrict__ cell_cnt, int32_t* __restrict__ cell_of,
                                                            int32_t* __restrict__ rank) {
  const int64_t j = (int64_t)blockIdx.x * NN_THREADS + threadIdx.x;
  if (j >= M) return;
  const float px = y[3 * j], py = y[3 * j + 1], pz = y[3 * j + 2];
  int c = -1, r = 0;
  if (nn_finite3(px, py, pz)) {
    const float ih = g->inv_h;
    const int cx = nn_cell_index(nn_cell_coord(px, g->bmin[0], ih), g->res[0]);
    const int cy = nn_cell_index(nn_cell_coord(py, g->bmin[1], ih), g->res[1]);
    const int cz = nn_cell_index(nn_cell_coord(pz, g->bmin[2], ih), g->res[2]);
    c = (cz * g->res[1] + cy) * g->res[0] + cx;
    r = atomicAdd(&cell_cnt[c], 1);
    if (r == 0) atomicAdd(&g->n_occ, 1);   // exactly one point per occupied cell sees rank 0
  }
  cell_of[j] = c;
  rank[j] = r;
}

// exclusive offsets of the cells in place; entry ncells (a zero count) becomes the number of finite points
__global__ void __launch_bounds__(MC_SCAN_THREADS) k_nn_scan(const NnGrid* __restrict__ g, int32_t* __restrict__ cell_cnt) {
  __shared__ int wtot[MC_SCAN_THREADS / 64];
  block_excl_scan_inplace(cell_cnt, (int64_t)g->ncells + 1, -1, nullptr, wtot);
}

__global__ void __launch_bounds__(NN_THREADS) k_nn_grid_fill(const float* __restrict__ y, int64_t M, const int32_t* __restrict__ cell_off,
                                                           const int32_t* __restrict__ cell_of, const int32_t* __restrict__ rank,
                                                           NnRec* __restrict__ rec) {
  const int64_t j = (int64_t)blockIdx.x * NN_THREADS + threadIdx.x;
  if (j >= M) return;
  const int c = cell_of[j];
  if (c < 0) return;
  NnRec v;
  v.x = y[3 * j];
  v.y = y[3 * j + 1];
  v.z = y[3 * j + 2];
  v.j = (int32_t)j;
  rec[cell_off[c] + rank[j]] = v;
}

__device__ __forceinline__ void nn_scan_records(const NnRec* __restrict__ rec, int p0, int p1, float qx, float qy, float qz, float& best,
                                                int& bi) {
  for (int p = p0; p < p1; ++p) {
    const NnRec v = rec[p];
    const float d = nn_dist2(qx, qy, qz, v.x, v.y, v.z);
    if (nn_better(d, v.j, best, bi)) {
      best = d;
      bi = v.j;
    }
  }
}

// Lower bound, in cells, of the distance along one axis from the query (cell coordinate u) to any point of y on the far side of
// the cell plane k (a point whose cell index is >= k when upper, < k when not).
//
// Why it is conservative.  Let t = nn_cell_coord(p) for such a point: t >= k (upper; the index is floor(t) clamped from above to
// res - 1 >= k) or 0 <= t < k (lower).  With a = p - bmin exactly, t = a (1 + d1)(1 + d2) inv_h, |d1|, |d2| <= eps = 2^-24 (one
// rounded subtraction, one rounded product), so a = t H / ((1 + d1)(1 + d2)) with H = 1 / inv_h, and the same for the query with
// u, wherever it lies (u < 0 or u > res outside the box).  Hence, upper side,
//     p - q >= H (t - u) - 2.01 eps H (|t| + |u|) >= H ((k - u) - 2.01 eps (k + |u|))
// (the middle expression grows with t), and the mirror image on the lower side.  The slack below, 2^-20 (k + |u| + 1), is 8
// times that plus the rounding of k - u itself; a non-positive or NaN gap (query beyond the plane, or u = +-inf for a query so far
// away that its coordinate overflows) gives 0: keep searching.
__device__ __forceinline__ float nn_plane_gap(float u, int k, bool upper) {
  const float kf = (float)k;
  const float gap = (upper ? kf - u : u - kf) - 9.5367431640625e-07f * (kf + fabsf(u) + 1.f);
  return gap > 0.f ? gap : 0.f;
}

// One thread per query: the cells at Chebyshev distance 0, 1, 2, ... from the query's (clamped) cell, clipped to the grid; a
// ring's interior rows contribute their two end cells, its border rows a contiguous run of records (x is the fastest cell
// index).  After ring r every unvisited point lies beyond one of the up to six planes of the visited box that are inside the
// grid (a clipped side has no cells, hence no points, beyond it -- this is also what makes a query outside y's box safe: its
// clamped cell sits on the grid's border, the side it lies beyond is clipped from r = 0, and the planes that remain are
// bounded through nn_plane_gap with the query's true, unclamped coordinate).  So every unvisited point is at least
// b = h_lo min(gaps) away, h_lo = h (1 - 2^-18) <= 1 / inv_h, and the search stops when best < b b STRICTLY: a point at
// exactly that distance could tie and carry a lower index.  The factor 1 - 2^-18 also covers the rounding of the computed
// distances (an unvisited point's computed d2 is at least its true value times 1 - 5 eps, and b b is rounded twice), and b b
// below 1e-30 counts as 0 (squares that underflow).  All sides clipped: the whole grid was read, done.  A query still open
// after max_rings rings is appended to left_list (integer atomic; the list's order is arbitrary, its content is not) and
// finished by k_nn_brute over all of y, which overwrites its outputs.
__global__ void __launch_bounds__(NN_THREADS) k_nn_grid_query(const float* __restrict__ x, int64_t N, const NnRec* __restrict__ rec,
                                                            const int32_t* __restrict__ cell_off, NnGrid* __restrict__ g, int max_rings,
                                                            float* __restrict__ d2, int32_t* __restrict__ idx,
                                                            int32_t* __restrict__ left_list) {
  const int64_t i = (int64_t)blockIdx.x * NN_THREADS + threadIdx.x;
  if (i >= N) return;
  const float q[3] = {x[3 * i], x[3 * i + 1], x[3 * i + 2]};
  float best = INFINITY;
  int bi = -1;
  bool done = !nn_finite3(q[0], q[1], q[2]) || g->n_finite == 0;
  // A few far outliers in y blow up the box, the cell budget then forces cells that hold the whole sweep, and walking such a
  // cell record by record per thread is an exhaustive search without the LDS tiles: when the occupied cells hold more than
  // NN_COARSE_FACTOR times the occupancy aimed at, every query goes to the tiled exhaustive pass instead.
  const bool coarse = (float)g->n_finite > NN_COARSE_FACTOR * g->target_occ * (float)g->n_occ;
  if (!done && coarse) {
    left_list[atomicAdd(&g->n_left, 1)] = (int32_t)i;
    done = true;
  }
  if (!done) {
    const int res[3] = {g->res[0], g->res[1], g->res[2]};
    const float ih = g->inv_h, h_lo = g->h * 0.999996185302734375f;
    float u[3];
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      u[a] = nn_cell_coord(q[a], g->bmin[a], ih);
      c[a] = nn_cell_index(u[a], res[a]);
    }
    for (int r = 0; r <= max_rings && !done; ++r) {
      int lo[3], hi[3], l[3], m[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        lo[a] = c[a] - r;
        hi[a] = c[a] + r;
        l[a] = lo[a] > 0 ? lo[a] : 0;
        m[a] = hi[a] < res[a] - 1 ? hi[a] : res[a] - 1;
      }
      for (int cz = l[2]; cz <= m[2]; ++cz)
        for (int cy = l[1]; cy <= m[1]; ++cy) {
          const int row = (cz * res[1] + cy) * res[0];
          if (cz == lo[2] || cz == hi[2] || cy == lo[1] || cy == hi[1]) {
            nn_scan_records(rec, cell_off[row + l[0]], cell_off[row + m[0] + 1], q[0], q[1], q[2], best, bi);
          } else {
            if (lo[0] >= 0) nn_scan_records(rec, cell_off[row + lo[0]], cell_off[row + lo[0] + 1], q[0], q[1], q[2], best, bi);
            if (hi[0] < res[0]) nn_scan_records(rec, cell_off[row + hi[0]], cell_off[row + hi[0] + 1], q[0], q[1], q[2], best, bi);
          }
        }
      float gap = INFINITY;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if (lo[a] >= 1) gap = fminf(gap, nn_plane_gap(u[a], lo[a], false));
        if (hi[a] + 1 <= res[a] - 1) gap = fminf(gap, nn_plane_gap(u[a], hi[a] + 1, true));
      }
      if (gap == INFINITY) {
        done = true;
      } else {
        const float b = gap * h_lo;
        float b2 = b * b;
        if (!(b2 > 1e-30f)) b2 = 0.f;
        done = best < b2;
      }
    }
    if (!done) left_list[atomicAdd(&g->n_left, 1)] = (int32_t)i;
  }
  d2[i] = best;
  idx[i] = bi;
}

// grid (query blocks, chunks of y).  qlist == NULL: queries 0 .. N - 1; else qlist[0 .. *nq_ptr).
__global__ void __launch_bounds__(NN_THREADS) k_nn_brute(const float* __restrict__ x, int64_t N, const float* __restrict__ y, int64_t M,
                                                       const int32_t* __restrict__ qlist, const int32_t* __restrict__ nq_ptr,
                                                       int64_t chunk, float* __restrict__ part_d2, int32_t* __restrict__ part_idx,
                                                       float* __restrict__ d2, int32_t* __restrict__ idx) {
  __shared__ __attribute__((aligned(16))) float sy[3][NN_TILE];
  int64_t nq = N;
  if (qlist) {
    const int64_t n = *nq_ptr;
    nq = n < N ? n : N;
  }
  const int tid = threadIdx.x;
  // query blocks in a grid-stride loop (block-uniform bounds): a launch for a list of unknown length stays small
  for (int64_t qblk = blockIdx.x; qblk * NN_THREADS < nq; qblk += gridDim.x) {
    const int64_t slot = qblk * NN_THREADS + tid;
    const bool active = slot < nq;
    const int64_t qi = !active ? 0 : qlist ? qlist[slot] : slot;
    const float qx = x[3 * qi], qy = x[3 * qi + 1], qz = x[3 * qi + 2];
    const int64_t j0 = (int64_t)blockIdx.y * chunk, j1 = (j0 + chunk) < M ? (j0 + chunk) : M;
    float best = INFINITY;
    int bi = -1;
    for (int64_t base = j0; base < j1; base += NN_TILE) {
      __syncthreads();
      for (int e = tid; e < 3 * NN_TILE; e += NN_THREADS) {   // coalesced [tile][3] -> three rows; NaN beyond the chunk
        const int64_t ge = 3 * base + e;
        sy[e % 3][e / 3] = ge < 3 * j1 ? y[ge] : NAN;
      }
      __syncthreads();
      const int64_t left = j1 - base;
      const int nt = left < NN_TILE ? (int)((left + 3) & ~(int64_t)3) : NN_TILE;
      for (int t = 0; t < nt; t += 4) {
        const nn_f4 px = *reinterpret_cast<const nn_f4*>(&sy[0][t]);
        const nn_f4 py = *reinterpret_cast<const nn_f4*>(&sy[1][t]);
        const nn_f4 pz = *reinterpret_cast<const nn_f4*>(&sy[2][t]);
        const float e0 = nn_dist2(qx, qy, qz, px.x, py.x, pz.x), e1 = nn_dist2(qx, qy, qz, px.y, py.y, pz.y);
        const float e2 = nn_dist2(qx, qy, qz, px.z, py.z, pz.z), e3 = nn_dist2(qx, qy, qz, px.w, py.w, pz.w);
        const int j = (int)(base + t);
        // ascending j: a strict < keeps the lowest index (nn_better's rule when j > bi)
        if (e0 < best) { best = e0; bi = j; }
        if (e1 < best) { best = e1; bi = j + 1; }
        if (e2 < best) { best = e2; bi = j + 2; }
        if (e3 < best) { best = e3; bi = j + 3; }
      }
    }
    if (active) {
      if (gridDim.y == 1) {
        d2[qi] = best;
        idx[qi] = bi;
      } else {
        part_d2[(int64_t)blockIdx.y * N + slot] = best;
        part_idx[(int64_t)blockIdx.y * N + slot] = bi;
      }
    }
  }
}

__global__ void __launch_bounds__(NN_THREADS) k_nn_combine(int64_t N, const int32_t* __restrict__ qlist, const int32_t* __restrict__ nq_ptr,
                                                         int nsplit, const float* __restrict__ part_d2,
                                                         const int32_t* __restrict__ part_idx, float* __restrict__ d2,
                                                         int32_t* __restrict__ idx) {
  int64_t nq = N;
  if (qlist) {
    const int64_t n = *nq_ptr;
    nq = n < N ? n : N;
  }
  const int64_t slot = (int64_t)blockIdx.x * NN_THREADS + threadIdx.x;
  if (slot >= nq) return;
  float best = INFINITY;
  int bi = -1;
  for (int s = 0; s < nsplit; ++s) {   // chunks ascend in j
    const float d = part_d2[(int64_t)s * N + slot];
    if (d < best) {
      best = d;
      bi = part_idx[(int64_t)s * N + slot];
    }
  }
  const int64_t qi = qlist ? qlist[slot] : slot;
  d2[qi] = best;
  idx[qi] = bi;
}

extern "C" {

int nsim_nn_brute(const float* x, int64_t N, const float* y, int64_t M, const int32_t* qlist, const int32_t* nq, int64_t nsplit,
                  float* part_d2, int32_t* part_idx, float* d2, int32_t* idx, void* stream) {
  if (N < 0 || M < 0 || nsplit < 1) return 2;
  if (N >= ((int64_t)1 << 31) - NN_TILE || M >= ((int64_t)1 << 31) - NN_TILE || nsplit > 65535) return 51;
  if (N == 0) return 0;
  if (!x || !d2 || !idx || (M > 0 && !y) || (qlist && !nq) || (nsplit > 1 && (!part_d2 || !part_idx))) return 4;
  // chunks of whole tiles; chunks that would be empty are not launched
  int64_t chunk = ((M + nsplit - 1) / nsplit + NN_TILE - 1) / NN_TILE * NN_TILE;
  if (chunk < NN_TILE) chunk = NN_TILE;
  int64_t ns = (M + chunk - 1) / chunk;
  if (ns < 1) ns = 1;
  const unsigned qb = (unsigned)((N + NN_THREADS - 1) / NN_THREADS);
  const unsigned qbl = (qlist && qb > NN_LIST_BLOCKS) ? NN_LIST_BLOCKS : qb;
  hipLaunchKernelGGL(k_nn_brute, dim3(qbl, (unsigned)ns), dim3(NN_THREADS), 0, (hipStream_t)stream, x, N, y, M, qlist, nq, chunk, part_d2,
                     part_idx, d2, idx);
  NSIM_CHECK_LAUNCH();
  if (ns > 1) {
    hipLaunchKernelGGL(k_nn_combine, dim3(qb), dim3(NN_THREADS), 0, (hipStream_t)stream, N, qlist, nq, (int)ns, part_d2, part_idx, d2,
                       idx);
    NSIM_CHECK_LAUNCH();
  }
  return 0;
}

int nsim_nn_grid_count(const float* y, int64_t M, float target_occ, int64_t max_cells, int32_t* hdr, int32_t* cell_cnt,
                       int32_t* cell_of, int32_t* rank, void* stream) {
  if (M < 0) return 2;
  if (M >= ((int64_t)1 << 31) - NN_TILE || max_cells < 1 || max_cells >= ((int64_t)1 << 30) || !(target_occ > 0.f)) return 51;
  if (!hdr || !cell_cnt || (M > 0 && (!y || !cell_of || !rank))) return 4;
  NnGrid* g = reinterpret_cast<NnGrid*>(hdr);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(hdr, 0, sizeof(NnGrid), st) != hipSuccess) return 1000;
  if (hipMemsetAsync(hdr, 0xff, 6 * sizeof(uint32_t), st) != hipSuccess) return 1000;
  if (hipMemsetAsync(cell_cnt, 0, (size_t)(max_cells + 1) * sizeof(int32_t), st) != hipSuccess) return 1000;
  if (M > 0) {
    hipLaunchKernelGGL(k_nn_bbox, dim3(nsim_blocks(M, NN_THREADS, 512)), dim3(NN_THREADS), 0, st, y, M, g);
    NSIM_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_nn_grid_setup, dim3(1), dim3(64), 0, st, g, target_occ, max_cells);
  NSIM_CHECK_LAUNCH();
  if (M > 0) {
    hipLaunchKernelGGL(k_nn_grid_count, dim3((unsigned)((M + NN_THREADS - 1) / NN_THREADS)), dim3(NN_THREADS), 0, st, y, M, g, cell_cnt,
                       cell_of, rank);
    NSIM_CHECK_LAUNCH();
  }
  return 0;
}

int nsim_nn_grid_scan(const int32_t* hdr, int32_t* cell_cnt, void* stream) {
  if (!hdr || !cell_cnt) return 4;
  hipLaunchKernelGGL(k_nn_scan, dim3(1), dim3(MC_SCAN_THREADS), 0, (hipStream_t)stream, reinterpret_cast<const NnGrid*>(hdr), cell_cnt);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_nn_grid_fill(const float* y, int64_t M, const int32_t* cell_off, const int32_t* cell_of, const int32_t* rank, float* rec,
                      void* stream) {
  if (M < 0) return 2;
  if (M == 0) return 0;
  if (!y || !cell_off || !cell_of || !rank || !rec) return 4;
  hipLaunchKernelGGL(k_nn_grid_fill, dim3((unsigned)((M + NN_THREADS - 1) / NN_THREADS)), dim3(NN_THREADS), 0, (hipStream_t)stream, y, M,
                     cell_off, cell_of, rank, reinterpret_cast<NnRec*>(rec));
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_nn_grid_query(const float* x, int64_t N, const float* rec, const int32_t* cell_off, int32_t* hdr, int max_rings, float* d2,
                       int32_t* idx, int32_t* left_list, void* stream) {
  if (N < 0 || max_rings < 0) return 2;
  if (N == 0) return 0;
  if (!x || !rec || !cell_off || !hdr || !d2 || !idx || !left_list) return 4;
  hipLaunchKernelGGL(k_nn_grid_query, dim3((unsigned)((N + NN_THREADS - 1) / NN_THREADS)), dim3(NN_THREADS), 0, (hipStream_t)stream, x, N,
                     reinterpret_cast<const NnRec*>(rec), cell_off, reinterpret_cast<NnGrid*>(hdr), max_rings, d2, idx, left_list);
  NSIM_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ occupancy grids
// code_single/tools/extract_occgrid.py:93-147, the kernels behind neuralsim_amd/occgrid.py.
//
// A voxel grid of resolution res[3] is classified from SDF values on the lattice its voxels SHARE: voxel (ix, iy, iz) has the
// (s + 1)^3 sample points of per-axis lattice indices i s .. i s + s, and the lattice has res[a] s + 1 points per axis.  A
// lattice tensor is f32 [LX][LY][LZ] (z fastest: voxels then come out in ascending (ix, iy, iz), torch.nonzero's order on an
// [X, Y, Z] array, whatever the slab cut) and is walked in slabs of nxs voxel layers in x = nxs s + 1 lattice planes.
//   * coordinates (k_og_points): lattice index j sits at c = float(j / s) + float(j % s) / float(s), cn = (c / float(res)) * 2 - 1,
//     x_world = cn * radius + center, x_obj[a] = ((R[0][a] d0 + R[1][a] d1) + R[2][a] d2) / scale[a] with d = x_world - t:
//     every operation rounds on its own (no contraction, IEEE division), as the separate tensor operations of the tool do, and
//     index i with k = s and index i + 1 with k = 0 name the same float, so both owners of a shared point see the same bits;
//   * state of a point: 0 = inside the object box (queried), 1 = outside (the tool's +inf), 2 = pruned: inside, but the cell
//     of the model's occupancy grid that contains it and its 26 neighbours (clamped at the border) are all empty;
//   * classification: pos = value > 0 (0, -0 and NaN are not positive), bad = isinf(value) or state != 0; a voxel is occupied
//     iff some sample is positive, some sample is not, and none is bad.  A pruned point has NO sign: its voxels are empty;
//   * three predicates that are all ORs, so the reduction is separable: k_og_flags ORs them over the (s + 1)^2 points in y and z
//     (a lattice value is read by at most 4 threads), one byte per (lattice plane, iy, iz); k_og_count / k_og_emit OR s + 1 of
//     those bytes along x;
//   * no atomics: counts per block of 256 voxels -> one scan (block_excl_scan_inplace) -> emission at the scanned offsets.
#define OG_STATE_OUT 1
#define OG_STATE_PRUNED 2

__device__ __forceinline__ int og_clamp(int c, int res) { return c < 0 ? 0 : (c > res - 1 ? res - 1 : c); }

__device__ __forceinline__ float og_coord(int64_t j, int s, int res) {
#pragma clang fp contract(off)
  const float c = (float)(j / s) + (float)(j % s) / (float)s;
  const float u = c / (float)res;
  const float v = u * 2.0f;
  return v - 1.0f;
}

__global__ void __launch_bounds__(MC_THREADS) k_og_points(NsimOccgridFrame f, int64_t j0, int64_t npts, int64_t ly, int64_t lz,
                                                        const uint32_t* __restrict__ bits, OccDev occ, float* __restrict__ x_obj,
                                                        uint8_t* __restrict__ state) {
#pragma clang fp contract(off)
  const int64_t q = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  if (q >= npts) return;
  const int64_t jz = q % lz, jy = (q / lz) % ly, jx = j0 + q / (lz * ly);
  const int64_t jj[3] = {jx, jy, jz};
  float d[3], xo[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float cn = og_coord(jj[a], f.s, f.res[a]);
    const float m = cn * f.radius[a];
    const float xw = m + f.center[a];
    d[a] = xw - f.trans[a];
  }
  bool inside = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float p0 = f.rot[0 + a] * d[0], p1 = f.rot[3 + a] * d[1], p2 = f.rot[6 + a] * d[2];
    const float s01 = p0 + p1;
    const float r = s01 + p2;
    xo[a] = r / f.scale[a];
    x_obj[3 * q + a] = xo[a];
    inside = inside && xo[a] >= f.obj_min[a] && xo[a] <= f.obj_max[a];
  }
  int st = inside ? 0 : OG_STATE_OUT;
  if (inside && bits) {
    int g[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float gf = floorf((xo[a] - occ.mn[a]) * occ.sc[a]);
      g[a] = gf >= (float)(occ.res[a] - 1) ? occ.res[a] - 1 : (gf > 0.f ? (int)gf : 0);      // a point on the upper face: last cell
    }
    bool any = false;
    for (int dz = -1; dz <= 1; ++dz)
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int cx = og_clamp(g[0] + dx, occ.res[0]), cy = og_clamp(g[1] + dy, occ.res[1]), cz = og_clamp(g[2] + dz, occ.res[2]);
          const int64_t flat = (int64_t)cx + (int64_t)occ.res[0] * ((int64_t)cy + (int64_t)occ.res[1] * (int64_t)cz);
          any = any || ((bits[flat >> 5] >> (flat & 31)) & 1u);
        }
    if (!any) st = OG_STATE_PRUNED;
  }
  state[q] = (uint8_t)st;
}

struct OgSlab {
  int64_t nxs, ry, rz;   // voxel layers of the slab in x, voxels in y and z
  int64_t ly, lz;        // lattice points in y and z
  int s;
};

// flags [nxs s + 1][ry][rz]: bit 0 = a positive sample, bit 1 = a sample that is not positive, bit 2 = a bad sample
__global__ void __launch_bounds__(MC_THREADS) k_og_flags(OgSlab g, const float* __restrict__ lat, const uint8_t* __restrict__ state,
                                                       uint8_t* __restrict__ flags) {
  const int64_t n = (g.nxs * g.s + 1) * g.ry * g.rz;
  const int64_t p = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  if (p >= n) return;
  const int64_t iz = p % g.rz, iy = (p / g.rz) % g.ry, jx = p / (g.rz * g.ry);
  int f = 0;
  for (int dy = 0; dy <= g.s; ++dy)
    for (int dz = 0; dz <= g.s; ++dz) {
      const int64_t q = (jx * g.ly + (iy * g.s + dy)) * g.lz + (iz * g.s + dz);
      if (state && state[q] != 0) {
        f |= 4;            // its value was never written: not read
        continue;
      }
      const float v = lat[q];
      f |= (v > 0.f ? 1 : 2) | (isinf(v) ? 4 : 0);
    }
  flags[p] = (uint8_t)f;
}

__device__ __forceinline__ int og_occupied(const OgSlab& g, const uint8_t* __restrict__ flags, int64_t p, int64_t& ix, int64_t& iy,
                                           int64_t& iz) {
  const int64_t plane = g.ry * g.rz, rem = p % plane;
  ix = p / plane;
  iy = rem / g.rz;
  iz = rem % g.rz;
  int f = 0;
  for (int dx = 0; dx <= g.s; ++dx) f |= flags[(ix * g.s + dx) * plane + rem];
  return f == 3 ? 1 : 0;
}

__global__ void __launch_bounds__(MC_THREADS) k_og_count(OgSlab g, const uint8_t* __restrict__ flags, int32_t* __restrict__ cnt) {
  __shared__ int wsum[MC_THREADS / 64][1];
  const int64_t p = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  int64_t ix, iy, iz;
  const int c[1] = {p < g.nxs * g.ry * g.rz ? og_occupied(g, flags, p, ix, iy, iz) : 0};
  int pre[1], tot[1];
  mc_block_scan<1>(c, pre, tot, wsum);
  if (threadIdx.x == 0) cnt[blockIdx.x] = tot[0];
}

// exclusive scan of the block counts in place; the total to *total and, if given, (total, seq) to the host-mapped notify words
__global__ void __launch_bounds__(MC_SCAN_THREADS) k_og_scan(int32_t* __restrict__ cnt, int64_t n, int32_t* __restrict__ total,
                                                           int64_t* notify, int64_t seq) {
  __shared__ int wtot[MC_SCAN_THREADS / 64];
  const int carry = block_excl_scan_inplace(cnt, n, -1, nullptr, wtot);
  if (threadIdx.x == 0) {
    *total = carry;
    if (notify) {
      nsim_store_system(notify, (int64_t)carry, false);
      nsim_store_system(notify + 1, seq, true);
    }
  }
}

__global__ void __launch_bounds__(MC_THREADS) k_og_emit(OgSlab g, const uint8_t* __restrict__ flags, int64_t ix0,
                                                      const int32_t* __restrict__ off, int32_t* __restrict__ out) {
  __shared__ int wsum[MC_THREADS / 64][1];
  const int64_t p = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  int64_t ix = 0, iy = 0, iz = 0;
  const int c[1] = {p < g.nxs * g.ry * g.rz ? og_occupied(g, flags, p, ix, iy, iz) : 0};
  int pre[1], tot[1];
  mc_block_scan<1>(c, pre, tot, wsum);
  if (!c[0]) return;
  const int64_t o = (int64_t)off[blockIdx.x] + pre[0];
  out[3 * o + 0] = (int32_t)(ix0 + ix);
  out[3 * o + 1] = (int32_t)iy;
  out[3 * o + 2] = (int32_t)iz;
}

// 56 unless 1 <= s <= 4 and the slab's voxels and lattice points both stay below 2^31
static int og_slab(int64_t nxs, int64_t ry, int64_t rz, int s, OgSlab& g) {
  if (nxs < 1 || ry < 1 || rz < 1) return 2;
  if (s < 1 || s > 4) return 56;
  const int64_t lim = (int64_t)1 << 31;
  if (nxs >= lim || ry >= lim || rz >= lim) return 56;
  g.nxs = nxs;
  g.ry = ry;
  g.rz = rz;
  g.ly = ry * s + 1;
  g.lz = rz * s + 1;
  g.s = s;
  if ((double)(nxs * s + 1) * (double)g.ly * (double)g.lz >= (double)lim) return 56;
  return 0;
}

extern "C" {

int nsim_occgrid_points(const NsimOccgridFrame* frame, int64_t j0, int64_t n_planes, const int32_t* occ_bits, const NsimOccMeta* occ,
                        float* x_obj, uint8_t* state, void* stream) {
  if (!frame) return 5;
  if (n_planes < 0 || j0 < 0) return 2;
  const int s = frame->s;
  if (s < 1 || s > 4) return 56;
  for (int a = 0; a < 3; ++a)
    if (frame->res[a] < 1 || (int64_t)frame->res[a] * s + 1 >= ((int64_t)1 << 24)) return 56;   // float(index) stays exact
  const int64_t ly = (int64_t)frame->res[1] * s + 1, lz = (int64_t)frame->res[2] * s + 1;
  if (j0 + n_planes > (int64_t)frame->res[0] * s + 1) return 56;
  if ((double)n_planes * (double)ly * (double)lz >= 2147483648.0) return 56;
  if (n_planes == 0) return 0;
  if (!x_obj || !state) return 4;
  if (occ_bits && !occ) return 5;
  OccDev od;
  memset(&od, 0, sizeof(od));
  if (occ_bits) {
    od = occ_dev(occ);
    for (int a = 0; a < 3; ++a)
      if (od.res[a] < 1) return 5;
  }
  const int64_t npts = n_planes * ly * lz;
  hipLaunchKernelGGL(k_og_points, dim3((unsigned)((npts + MC_THREADS - 1) / MC_THREADS)), dim3(MC_THREADS), 0, (hipStream_t)stream,
                     *frame, j0, npts, ly, lz, reinterpret_cast<const uint32_t*>(occ_bits), od, x_obj, state);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_occgrid_flags(const float* lat, const uint8_t* state, int64_t nxs, int64_t ry, int64_t rz, int s, uint8_t* flags,
                       void* stream) {
  OgSlab g;
  const int rc = og_slab(nxs, ry, rz, s, g);
  if (rc) return rc;
  if (!lat || !flags) return 4;
  const int64_t n = (nxs * s + 1) * ry * rz;
  hipLaunchKernelGGL(k_og_flags, dim3((unsigned)((n + MC_THREADS - 1) / MC_THREADS)), dim3(MC_THREADS), 0, (hipStream_t)stream, g, lat,
                     state, flags);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_occgrid_count(const uint8_t* flags, int64_t nxs, int64_t ry, int64_t rz, int s, int32_t* cnt, void* stream) {
  OgSlab g;
  const int rc = og_slab(nxs, ry, rz, s, g);
  if (rc) return rc;
  if (!flags || !cnt) return 4;
  const int64_t n = nxs * ry * rz;
  hipLaunchKernelGGL(k_og_count, dim3((unsigned)((n + MC_THREADS - 1) / MC_THREADS)), dim3(MC_THREADS), 0, (hipStream_t)stream, g, flags,
                     cnt);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_occgrid_scan(int32_t* cnt, int64_t n_blocks, int32_t* total, int64_t* notify, int64_t seq, void* stream) {
  if (n_blocks < 1) return 2;
  if (!cnt || !total) return 4;
  hipLaunchKernelGGL(k_og_scan, dim3(1), dim3(MC_SCAN_THREADS), 0, (hipStream_t)stream, cnt, n_blocks, total, notify, seq);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_occgrid_emit(const uint8_t* flags, int64_t nxs, int64_t ry, int64_t rz, int s, int64_t ix0, const int32_t* off, int32_t* out,
                      void* stream) {
  OgSlab g;
  const int rc = og_slab(nxs, ry, rz, s, g);
  if (rc) return rc;
  if (ix0 < 0 || ix0 + nxs >= ((int64_t)1 << 31)) return 56;
  if (!flags || !off || !out) return 4;
  const int64_t n = nxs * ry * rz;
  hipLaunchKernelGGL(k_og_emit, dim3((unsigned)((n + MC_THREADS - 1) / MC_THREADS)), dim3(MC_THREADS), 0, (hipStream_t)stream, g, flags,
                     ix0, off, out);
  NSIM_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ visible grids
// app/visible_grid.py and code_multi/tools/extract_visible_grid.py:205-235, the kernels behind neuralsim_amd/visible_grid.py.
//
// The grid is the cube [origin, origin + G voxel] of G^3 voxels, G = 2^octree_depth (32 .. 1024); a voxel's index is the
// reference's ix G G + iy G + iz (z fastest) in int64 -- 2^30 voxels occur.  The working state is two dense arrays in that order:
// hits int32 [G^3] (samples seen per voxel, summed over all calls) and bit sets uint32 [G^3 / 32] (bit v & 31 of word v >> 5).
//   * a point counts iff box_min <= p <= box_max on every axis (``space.contains``; NaN is outside); its voxel coordinate is
//     int((p - origin) / voxel) clamped to G - 1 (a point on the upper face of the longest axis), every operation rounded on
//     its own and the division IEEE, as the separate tensor operations of the reference are (vg_voxel);
//   * marking (k_vg_mark_samples: p = o + d t of the samples with w > thre -- strict, NaN is not greater -- one thread per sample,
//     its pack found by bisection over the pack starts; k_vg_mark_points: a plain point array): consecutive samples of a ray
//     sit in consecutive lanes and share voxels, and same-address atomics are separate requests at the memory side, so runs
//     of equal voxels are merged in the wave (the ballot / run-head scheme of occ_max_wave, occ_dev.h) and the head lane of a
//     run issues ONE integer atomicAdd(hits[v], run length).  Integer adds commute: the counts do not depend on the order;
//   * k_vg_morph: out = op(in) | keep, op = 3x3x3 box dilation (out-of-grid neighbours dropped) or erosion (out-of-grid
//     neighbours empty), one thread per 32-voxel word: z neighbours by shifts with the carry from the adjacent word of the
//     SAME row (x, y) only, x and y neighbours from the 8 neighbouring rows;
//   * compaction without atomics: set bits per block of 256 words (k_vg_count) -> nsim_occgrid_scan -> k_vg_emit writes the
//     indices in storage order = ascending, and the hit counts gathered at them;
//   * k_vg_occ_val: the accel's value grid (x fastest, sampling.hip) = 1.0 where the bit is set, else 0.0 -- the one
//     transposition between the two voxel orders, in tiles of 32 (x) by 32 (z) through shared memory after a memset.
#define VG_DILATE 0
#define VG_ERODE 1

__device__ __forceinline__ bool vg_voxel(const NsimVgridFrame& f, float px, float py, float pz, int64_t& flat) {
#pragma clang fp contract(off)
  const float p[3] = {px, py, pz};
  bool in = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) in = in && p[a] >= f.box_min[a] && p[a] <= f.box_max[a];
  if (!in) return false;
  int64_t c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float d = p[a] - f.origin[a];
    const float q = d / f.voxel[a];
    c[a] = q >= (float)(f.G - 1) ? f.G - 1 : (q > 0.f ? (int)q : 0);
  }
  flat = (c[0] * f.G + c[1]) * f.G + c[2];
  return true;
}

// hits[flat] += 1 for the lanes with ``ok`` (all 64 lanes call): one atomicAdd of the run length per run of equal voxels
__device__ __forceinline__ void vg_mark_wave(int32_t* __restrict__ hits, bool ok, int64_t flat_in, unsigned long long* stats) {
  const int lane = nsim_lane();
  const int64_t flat = ok ? flat_in : (int64_t)(-1 - lane);
  const int64_t pk = wave_shfl(flat, lane - 1);
  const unsigned long long heads = wave_ballot(lane == 0 || pk != flat);
  const unsigned long long kept = wave_ballot(ok);
  if (ok && ((heads >> lane) & 1ull)) {
    const unsigned long long above = lane == 63 ? 0ull : (heads >> (lane + 1));
    const int len = above ? __builtin_ctzll(above) + 1 : 64 - lane;
    atomicAdd(hits + flat, len);
  }
  if (stats && lane == 0 && kept) {      // (bench only) kept samples and atomics issued
    atomicAdd(stats, (unsigned long long)__popcll(kept));
    atomicAdd(stats + 1, (unsigned long long)__popcll(heads & kept));
  }
}

__global__ void __launch_bounds__(MC_THREADS) k_vg_mark_samples(NsimVgridFrame f, const float* __restrict__ rays_o,
                                                              const float* __restrict__ rays_d, int64_t n_rays,
                                                              const int64_t* __restrict__ rays_inds,
                                                              const int64_t* __restrict__ pack_infos, int64_t n_packs,
                                                              const float* __restrict__ t, const float* __restrict__ w, int64_t S,
                                                              float thre, int32_t* __restrict__ hits, unsigned long long* stats) {
#pragma clang fp contract(off)
  const int64_t s = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  bool ok = s < S;
  int64_t flat = 0;
  if (ok) ok = w[s] > thre;
  if (ok) {
    int64_t lo = 0, hi = n_packs;            // the first pack that starts after s
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (pack_infos[2 * mid] <= s) lo = mid + 1; else hi = mid;
    }
    const int64_t p = lo - 1;
    ok = p >= 0 && s < pack_infos[2 * p] + pack_infos[2 * p + 1];
    int64_t r = 0;
    if (ok) {
      r = rays_inds ? rays_inds[p] : p;
      ok = r >= 0 && r < n_rays;
    }
    if (ok) {
      const float tt = t[s];
      float x[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float m = rays_d[3 * r + a] * tt;
        x[a] = rays_o[3 * r + a] + m;
      }
      ok = vg_voxel(f, x[0], x[1], x[2], flat);
    }
  }
  vg_mark_wave(hits, ok, flat, stats);
}

__global__ void __launch_bounds__(MC_THREADS) k_vg_mark_points(NsimVgridFrame f, const float* __restrict__ pts, int64_t n,
                                                             int32_t* __restrict__ hits, unsigned long long* stats) {
  const int64_t i = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  bool ok = i < n;
  int64_t flat = 0;
  if (ok) ok = vg_voxel(f, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], flat);
  vg_mark_wave(hits, ok, flat, stats);
}

// nvox is a multiple of 64: every wave is whole
__global__ void __launch_bounds__(MC_THREADS) k_vg_bits(const int32_t* __restrict__ hits, int64_t nvox, uint32_t* __restrict__ bits) {
  const int64_t v = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  const int lane = nsim_lane();
  const unsigned long long b = wave_ballot(v < nvox && hits[v] > 0);
  if (v < nvox && (lane & 31) == 0) bits[v >> 5] = (uint32_t)(b >> (lane & 32));
}

__global__ void __launch_bounds__(MC_THREADS) k_vg_set_bits(const int64_t* __restrict__ idx, int64_t n, int64_t nvox,
                                                          uint32_t* __restrict__ bits) {
  const int64_t i = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  if (i >= n) return;
  const int64_t v = idx[i];
  if (v < 0 || v >= nvox) return;
  atomicOr(bits + (v >> 5), 1u << (v & 31));
}

__global__ void __launch_bounds__(MC_THREADS) k_vg_morph(const uint32_t* __restrict__ in, const uint32_t* keep, int64_t G, int op,
                                                       uint32_t* out) {
  const int64_t W = G >> 5, nw = G * G * W;
  const int64_t w = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  if (w >= nw) return;
  const int64_t wz = w % W, y = (w / W) % G, x = w / (W * G);
  uint32_t acc = op == VG_DILATE ? 0u : in[w];
  if (op == VG_DILATE || acc != 0u)
    for (int dx = -1; dx <= 1; ++dx)
      for (int dy = -1; dy <= 1; ++dy) {
        const int64_t xx = x + dx, yy = y + dy;
        if (xx < 0 || xx >= G || yy < 0 || yy >= G) {
          if (op == VG_ERODE) acc = 0u;
          continue;
        }
        const int64_t base = (xx * G + yy) * W;
        const uint32_t c = in[base + wz];
        const uint32_t l = wz > 0 ? in[base + wz - 1] : 0u;          // the carries stay inside the row
        const uint32_t r = wz + 1 < W ? in[base + wz + 1] : 0u;
        const uint32_t up = (c << 1) | (l >> 31);                    // bit z = voxel z - 1
        const uint32_t dn = (c >> 1) | (r << 31);                    // bit z = voxel z + 1
        if (op == VG_DILATE) acc |= c | up | dn; else acc &= c & up & dn;
      }
  out[w] = acc | (keep ? keep[w] : 0u);
}

// exclusive prefix of c (0 .. 32 set bits of a word: mc_block_scan's ballot scan takes values below 8) among the block's threads
// and the block total
__device__ __forceinline__ void vg_block_scan(int c, int& pre, int& tot, int* wsum) {
  const int lane = nsim_lane(), wave = threadIdx.x >> 6;
  int inc = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = wave_shfl(inc, lane - d);
    if (lane >= d) inc += o;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < MC_THREADS / 64; ++w) {
    before += w < wave ? wsum[w] : 0;
    all += wsum[w];
  }
  pre = inc - c + before;
  tot = all;
}

__global__ void __launch_bounds__(MC_THREADS) k_vg_count(const uint32_t* __restrict__ bits, int64_t nw, int32_t* __restrict__ cnt) {
  __shared__ int wsum[MC_THREADS / 64];
  const int64_t w = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  int pre, tot;
  vg_block_scan(w < nw ? (int)__popc(bits[w]) : 0, pre, tot, wsum);
  if (threadIdx.x == 0) cnt[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(MC_THREADS) k_vg_emit(const uint32_t* __restrict__ bits, int64_t nw, const int32_t* __restrict__ off,
                                                      const int32_t* __restrict__ hits, int64_t* __restrict__ out_idx,
                                                      int64_t* __restrict__ out_hits) {
  __shared__ int wsum[MC_THREADS / 64];
  const int64_t w = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  uint32_t b = w < nw ? bits[w] : 0u;
  int pre, tot;
  vg_block_scan((int)__popc(b), pre, tot, wsum);
  int64_t o = (int64_t)off[blockIdx.x] + pre;
  while (b) {
    const int k = __builtin_ctz(b);
    b &= b - 1u;
    const int64_t v = (w << 5) + k;
    out_idx[o] = v;
    if (out_hits) out_hits[o] = hits ? (int64_t)hits[v] : 0;
    ++o;
  }
}

// One block per tile of 32 voxels in x by one word (32 voxels) in z at one y: the 32 words (x0 .. x0 + 31, y, wz) are read once and
// the set bits written as rows of 32 consecutive floats in x.  The value grid was zeroed before: only set bits are written.
__global__ void __launch_bounds__(MC_THREADS) k_vg_occ_val(const uint32_t* __restrict__ bits, int64_t G, float* __restrict__ val) {
  __shared__ uint32_t wds[32];
  const int64_t W = G >> 5, b = blockIdx.x;
  const int64_t wz = b % W, y = (b / W) % G, x0 = (b / (W * G)) << 5;
  const int tid = threadIdx.x;
  if (tid < 32) wds[tid] = bits[((x0 + tid) * G + y) * W + wz];
  __syncthreads();
  const int x = tid & 31;
  const uint32_t wd = wds[x];
#pragma unroll
  for (int i = 0; i < 32 / (MC_THREADS / 32); ++i) {
    const int z = (tid >> 5) + (MC_THREADS / 32) * i;
    if ((wd >> z) & 1u) val[(x0 + x) + G * (y + G * ((wz << 5) + z))] = 1.0f;
  }
}

// 57 unless G is a power of two in 32 .. 1024
static int vg_grid(int64_t G) { return (G >= 32 && G <= 1024 && (G & (G - 1)) == 0) ? 0 : 57; }
static dim3 vg_blocks(int64_t n) { return dim3((unsigned)((n + MC_THREADS - 1) / MC_THREADS)); }

extern "C" {

int nsim_vgrid_mark_samples(const NsimVgridFrame* frame, const float* rays_o, const float* rays_d, int64_t n_rays,
                            const int64_t* rays_inds_hit, const int64_t* pack_infos_hit, int64_t n_packs, const float* t,
                            const float* w, int64_t S, float thre, int32_t* hits, int64_t* stats, void* stream) {
  if (!frame) return 5;
  const int rc = vg_grid(frame->G);
  if (rc) return rc;
  if (n_rays < 0 || n_packs < 0 || S < 0) return 2;
  if (S >= ((int64_t)1 << 39)) return 57;
  if (!hits) return 4;
  if (S == 0 || n_packs == 0 || n_rays == 0) return 0;
  if (!rays_o || !rays_d || !pack_infos_hit || !t || !w) return 24;
  hipLaunchKernelGGL(k_vg_mark_samples, vg_blocks(S), dim3(MC_THREADS), 0, (hipStream_t)stream, *frame, rays_o, rays_d, n_rays,
                     rays_inds_hit, pack_infos_hit, n_packs, t, w, S, thre, hits, reinterpret_cast<unsigned long long*>(stats));
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_vgrid_mark_points(const NsimVgridFrame* frame, const float* pts, int64_t n, int32_t* hits, int64_t* stats, void* stream) {
  if (!frame) return 5;
  const int rc = vg_grid(frame->G);
  if (rc) return rc;
  if (n < 0) return 2;
  if (n >= ((int64_t)1 << 39)) return 57;
  if (!hits) return 4;
  if (n == 0) return 0;
  if (!pts) return 24;
  hipLaunchKernelGGL(k_vg_mark_points, vg_blocks(n), dim3(MC_THREADS), 0, (hipStream_t)stream, *frame, pts, n, hits,
                     reinterpret_cast<unsigned long long*>(stats));
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_vgrid_bits(const int32_t* hits, int64_t G, int32_t* bits, void* stream) {
  const int rc = vg_grid(G);
  if (rc) return rc;
  if (!hits || !bits) return 4;
  hipLaunchKernelGGL(k_vg_bits, vg_blocks(G * G * G), dim3(MC_THREADS), 0, (hipStream_t)stream, hits, G * G * G,
                     reinterpret_cast<uint32_t*>(bits));
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_vgrid_set_bits(const int64_t* idx, int64_t n, int64_t G, int32_t* bits, void* stream) {
  const int rc = vg_grid(G);
  if (rc) return rc;
  if (n < 0) return 2;
  if (n > G * G * G) return 57;
  if (!bits) return 4;
  if (n == 0) return 0;
  if (!idx) return 24;
  hipLaunchKernelGGL(k_vg_set_bits, vg_blocks(n), dim3(MC_THREADS), 0, (hipStream_t)stream, idx, n, G * G * G,
                     reinterpret_cast<uint32_t*>(bits));
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_vgrid_morph(const int32_t* in, const int32_t* keep, int64_t G, int op, int32_t* out, void* stream) {
  const int rc = vg_grid(G);
  if (rc) return rc;
  if (op != VG_DILATE && op != VG_ERODE) return 3;
  if (!in || !out || in == out) return 4;
  hipLaunchKernelGGL(k_vg_morph, vg_blocks(G * G * (G >> 5)), dim3(MC_THREADS), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint32_t*>(in), reinterpret_cast<const uint32_t*>(keep), G, op,
                     reinterpret_cast<uint32_t*>(out));
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_vgrid_count(const int32_t* bits, int64_t G, int32_t* cnt, void* stream) {
  const int rc = vg_grid(G);
  if (rc) return rc;
  if (!bits || !cnt) return 4;
  const int64_t nw = G * G * (G >> 5);
  hipLaunchKernelGGL(k_vg_count, vg_blocks(nw), dim3(MC_THREADS), 0, (hipStream_t)stream, reinterpret_cast<const uint32_t*>(bits), nw,
                     cnt);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_vgrid_emit(const int32_t* bits, int64_t G, const int32_t* off, const int32_t* hits, int64_t* out_idx, int64_t* out_hits,
                    void* stream) {
  const int rc = vg_grid(G);
  if (rc) return rc;
  if (!bits || !off || !out_idx) return 4;
  const int64_t nw = G * G * (G >> 5);
  hipLaunchKernelGGL(k_vg_emit, vg_blocks(nw), dim3(MC_THREADS), 0, (hipStream_t)stream, reinterpret_cast<const uint32_t*>(bits), nw,
                     off, hits, out_idx, out_hits);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_vgrid_occ_val(const int32_t* bits, int64_t G, float* occ_val, void* stream) {
  const int rc = vg_grid(G);
  if (rc) return rc;
  if (!bits || !occ_val) return 4;
  const hipError_t e = hipMemsetAsync(occ_val, 0, (size_t)(G * G * G) * sizeof(float), (hipStream_t)stream);
  if (e != hipSuccess) return 1000 + (int)e;
  hipLaunchKernelGGL(k_vg_occ_val, dim3((unsigned)(G * G * G / 1024)), dim3(MC_THREADS), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint32_t*>(bits), G, occ_val);
  NSIM_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ simulated LiDAR returns
// The point cloud of a rendered sweep (code_multi/tools/render.py:331-346 and :298-313: a boolean mask and five to seven masked
// gathers), the kernels behind neuralsim_amd/lidar_sim.py.  A ray is a return iff acc[r] > thresh (strict, f32; NaN is not
// greater).  Compaction without atomics, in ray order: returns per block of 256 rays (k_lr_count) -> nsim_occgrid_scan ->
// k_lr_emit; the rank inside a wave is the popcount of the ballot below the lane.  Per return at output row o:
//   ray_inds[o] = r, ranges[o] = depth[r], mask[o] = acc[r], rgb / ids rows copied,
//   pts_world[o] = o_r + d_r * range          one multiply then one add per component (never fused),
//   pts_local[o][k] = ((m[k][0] x + m[k][1] y) + m[k][2] z) + m[k][3]    with (x, y, z) = pts_world[o], m = w2l [3,4].
// range_image [N] (optional, dense): depth[r] on a return, 0 elsewhere.
__device__ __forceinline__ int lr_block_rank(int c, int& tot, int* wsum) {
  const int lane = nsim_lane(), wave = threadIdx.x >> 6;
  const unsigned long long b = wave_ballot(c);
  if (lane == 0) wsum[wave] = __popcll(b);
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < MC_THREADS / 64; ++w) {
    before += w < wave ? wsum[w] : 0;
    all += wsum[w];
  }
  tot = all;
  return before + __popcll(b & ((1ull << lane) - 1ull));
}

__global__ void __launch_bounds__(MC_THREADS) k_lr_count(const float* __restrict__ acc, int64_t N, float thresh,
                                                       int32_t* __restrict__ cnt) {
  __shared__ int wsum[MC_THREADS / 64];
  const int64_t r = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  int tot;
  lr_block_rank(r < N && acc[r] > thresh ? 1 : 0, tot, wsum);
  if (threadIdx.x == 0) cnt[blockIdx.x] = tot;
}

struct LrOut {
  int64_t* ray_inds;
  float *ranges, *mask, *pts_world, *pts_local, *rgb;
  int64_t* ids;
  float* range_image;
};

__global__ void __launch_bounds__(MC_THREADS) k_lr_emit(const float* __restrict__ acc, const float* __restrict__ depth,
                                                      const float* __restrict__ rays_o, const float* __restrict__ rays_d, int64_t N,
                                                      float thresh, const int32_t* __restrict__ off, const float* __restrict__ w2l,
                                                      const float* __restrict__ rgb, const int64_t* __restrict__ ids, LrOut out) {
  __shared__ int wsum[MC_THREADS / 64];
  const int64_t r = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  const float a = r < N ? acc[r] : 0.f;
  const int c = r < N && a > thresh ? 1 : 0;
  int tot;
  const int rank = lr_block_rank(c, tot, wsum);
  if (r >= N) return;
  const float rg = depth[r];
  if (out.range_image) out.range_image[r] = c ? rg : 0.f;
  if (!c) return;
  const int64_t o = (int64_t)off[blockIdx.x] + rank;
  out.ray_inds[o] = r;
  out.ranges[o] = rg;
  out.mask[o] = a;
  float p[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float t = rays_d[3 * r + k] * rg;
    p[k] = rays_o[3 * r + k] + t;
    out.pts_world[3 * o + k] = p[k];
  }
  if (out.pts_local)
#pragma unroll
    for (int k = 0; k < 3; ++k) out.pts_local[3 * o + k] = ((w2l[4 * k] * p[0] + w2l[4 * k + 1] * p[1]) + w2l[4 * k + 2] * p[2]) + w2l[4 * k + 3];
  if (out.rgb)
#pragma unroll
    for (int k = 0; k < 3; ++k) out.rgb[3 * o + k] = rgb[3 * r + k];
  if (out.ids) out.ids[o] = ids[r];
}

extern "C" {

int nsim_lidar_returns_count(const float* acc, int64_t N, float thresh, int32_t* cnt, void* stream) {
  if (N < 0) return 2;
  if (N >= ((int64_t)1 << 31)) return 61;
  if (N == 0) return 0;
  if (!cnt) return 4;
  if (!acc) return 61;
  hipLaunchKernelGGL(k_lr_count, vg_blocks(N), dim3(MC_THREADS), 0, (hipStream_t)stream, acc, N, thresh, cnt);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_lidar_returns_emit(const float* acc, const float* depth, const float* rays_o, const float* rays_d, int64_t N, float thresh,
                            const int32_t* off, const float* w2l, const float* rgb, const int64_t* ids, int64_t* ray_inds,
                            float* ranges, float* mask, float* pts_world, float* pts_local, float* out_rgb, int64_t* out_ids,
                            float* range_image, void* stream) {
  if (N < 0) return 2;
  if (N >= ((int64_t)1 << 31)) return 61;
  if (N == 0) return 0;
  if (!ray_inds || !ranges || !mask || !pts_world) return 4;
  if (!acc || !depth || !rays_o || !rays_d || !off) return 61;
  if ((pts_local && !w2l) || (out_rgb && !rgb) || (out_ids && !ids)) return 61;
  LrOut out;
  out.ray_inds = ray_inds;
  out.ranges = ranges;
  out.mask = mask;
  out.pts_world = pts_world;
  out.pts_local = pts_local;
  out.rgb = out_rgb;
  out.ids = out_ids;
  out.range_image = range_image;
  hipLaunchKernelGGL(k_lr_emit, vg_blocks(N), dim3(MC_THREADS), 0, (hipStream_t)stream, acc, depth, rays_o, rays_d, N, thresh, off,
                     w2l, rgb, ids, out);
  NSIM_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ LiDAR ground-truth filter
// SceneDataLoader._filter_lidar_gts (dataio/data_loader/base_loader.py:732-844) on top of Camera.project_pts_in_image
// (app/resources/observers/cameras.py:397-446), the kernels behind neuralsim_amd/lidar_filter.py.  The reference applies four
// filters one after another, each a mask, a nonzero and a gather of every column; the rule is per point, so they are ONE
// conjunction here: k_lf_count writes keep u8 [N] and the kept points per block of 256 -> nsim_occgrid_scan -> k_lf_emit
// compacts the columns in point order (ranks from the ballot popcount, lr_block_rank).  Every product is rounded before its sum
// (-ffp-contract=off), every 3-term sum runs left to right:
//   p_local = o + d * range (one multiply, one add);  p[k] = ((R[k][0] x + R[k][1] y) + R[k][2] z) + t[k], (R, t) = l2w[fi][li];
//   a camera / box frame: q = p - t, b[k] = (R[0][k] q0 + R[1][k] q1) + R[2][k] q2 (the transposed rotation, no inverse);
//   (u, v, d) by lf_uvd, operation for operation the ``proj`` of the three camera models; in view iff d > near_clip and
//   0 <= u < W and 0 <= v < H; an ignore mask is read at [(int)v][(int)u] only after that test passed (outside the mask's
//   own extent a pixel counts as padding, 0).
// A camera record is LF_CAM floats: c2w [3][4], fx, skew, cx, fy, cy, W, H, five distortion coefficients; the model ids (one
// per camera of the rig, the same in every frame) travel as a launch argument, 2 bits each.  A block whose points share a
// frame (a frame-sorted bank: all but the blocks on a frame boundary) stages that frame's cameras and its boxes, LF_BOX_CHUNK
// at a time, in LDS; any other block reads the records of each point's own frame from global memory.  A point whose frame or
// lidar index is outside the tables is not kept (and reads nothing).
#define LF_CAM 24
#define LF_MAX_CAMS 32
#define LF_BOX 15
#define LF_BOX_CHUNK 64

struct LfPoses {
  const float* l2w;        // [F L][3][4]
  const int64_t *li, *fi;  // per point, may be NULL (0)
  int64_t L, F;
};

// -> false when the point's frame / lidar index is outside the tables
__device__ __forceinline__ bool lf_world_point(const LfPoses& ps, const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                               float range, int64_t r, int64_t& f, float p[3]) {
  f = ps.fi ? ps.fi[r] : 0;
  const int64_t l = ps.li ? ps.li[r] : 0;
  if (f < 0 || f >= ps.F || l < 0 || l >= ps.L) return false;
  float q[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float t = rays_d[3 * r + k] * range;
    q[k] = rays_o[3 * r + k] + t;
  }
  const float* m = ps.l2w + 12 * (f * ps.L + l);
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = ((m[4 * k] * q[0] + m[4 * k + 1] * q[1]) + m[4 * k + 2] * q[2]) + m[4 * k + 3];
  return true;
}

// b = R^T (p - t) of a row-major [3][4] transform m
__device__ __forceinline__ void lf_to_frame(const float* m, const float p[3], float b[3]) {
  const float q0 = p[0] - m[3], q1 = p[1] - m[7], q2 = p[2] - m[11];
#pragma unroll
  for (int k = 0; k < 3; ++k) b[k] = (m[k] * q0 + m[4 + k] * q1) + m[8 + k] * q2;
}

// camera-frame point -> (u, v, depth): nr3d_lib attributes ``proj`` of the pinhole (0), OpenCV (1) and fisheye (2) intrinsics
__device__ __forceinline__ void lf_uvd(const float* cam, int model, const float c[3], float& u, float& v, float& d) {
  const float fx = cam[12], sk = cam[13], cx = cam[14], fy = cam[15], cy = cam[16];
  const float* k = cam + 19;
  const float x = c[0], y = c[1], z = c[2];
  d = z;
  if (model == 2) {
    const float r = sqrtf(x * x + y * y);
    const float th = atan2f(r, z);
    const float t2 = th * th;
    const float thd = th * (1.0f + (((k[3] * t2 + k[2]) * t2 + k[1]) * t2 + k[0]) * t2);
    const float sc = r > 1e-12f ? thd / fmaxf(r, 1e-12f) : 1.0f;
    u = fx * (x * sc) + cx;
    v = fy * (y * sc) + cy;
    return;
  }
  const float zs = fabsf(z) < 1e-9f ? 1e-9f : z;
  if (model == 0) {
    u = ((fx * x) / zs + (sk * y) / zs) + cx;
    v = (fy * y) / zs + cy;
    return;
  }
  const float xn = x / zs, yn = y / zs;
  const float r2 = xn * xn + yn * yn;
  const float cd = 1.0f + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2;
  const float xd = (xn * cd + ((2.0f * k[2]) * xn) * yn) + k[3] * (r2 + (2.0f * xn) * xn);
  const float yd = (yn * cd + k[2] * (r2 + (2.0f * yn) * yn)) + ((2.0f * k[3]) * xn) * yn;
  u = (fx * xd + sk * yd) + cx;
  v = fy * yd + cy;
}

// THE view test, of the filter and of the dense projection alike.  ign: this camera's ignore plane [Hm][Wm] or NULL.
__device__ __forceinline__ bool lf_in_view(const float* cam, int model, const float p[3], float near_clip,
                                           const uint8_t* __restrict__ ign, int64_t Hm, int64_t Wm, float& u, float& v, float& d) {
  float c[3];
  lf_to_frame(cam, p, c);
  lf_uvd(cam, model, c, u, v, d);
  if (!(d > near_clip && u < cam[17] && u >= 0.f && v < cam[18] && v >= 0.f)) return false;
  if (ign) {
    const int64_t iu = (int64_t)u, iv = (int64_t)v;
    if (iu < Wm && iv < Hm && ign[iv * Wm + iu]) return false;
  }
  return true;
}

__device__ __forceinline__ bool lf_in_box(const float* box, const float p[3]) {
  float b[3];
  lf_to_frame(box, p, b);
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float h = box[12 + k] / 2.0f;
    in = in && b[k] >= -h && b[k] <= h;
  }
  return in;
}

struct LfRule {
  int filter_valid;
  const float* cams;       // [F C][LF_CAM] or NULL
  uint64_t models;         // 2 bits per camera
  int64_t C;
  float near_clip;
  const uint8_t* ignore;   // [F C][Hm][Wm] or NULL
  int64_t Hm, Wm;
  const float* aabb;       // [2][3] or NULL
  const float* boxes;      // [B][LF_BOX] or NULL
  const int32_t* box_off;  // [F + 1]
  int64_t B;
};

__global__ void __launch_bounds__(MC_THREADS) k_lf_count(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                       const float* __restrict__ ranges, int64_t N, LfPoses ps, LfRule rl,
                                                       uint8_t* __restrict__ keep, int32_t* __restrict__ cnt) {
  __shared__ int wsum[MC_THREADS / 64];
  __shared__ int mixed;
  __shared__ float s_cam[LF_MAX_CAMS * LF_CAM];
  __shared__ float s_box[LF_BOX_CHUNK * LF_BOX];
  const int tid = threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x * MC_THREADS + tid;
  const int64_t r0 = (int64_t)blockIdx.x * MC_THREADS;
  const int64_t f0 = ps.fi ? ps.fi[r0] : 0;        // the block's frame, if it has one (r0 < N for every launched block)
  if (tid == 0) mixed = 0;
  __syncthreads();
  float p[3] = {0.f, 0.f, 0.f};
  int64_t f = 0;
  bool live = false;
  if (r < N) {
    const float rg = ranges[r];
    live = lf_world_point(ps, rays_o, rays_d, rg, r, f, p);
    if (ps.fi && ps.fi[r] != f0) mixed = 1;         // (an index outside the table as well: f0 may be such a one)
    if (rl.filter_valid && !(rg > 0.f)) live = false;
    if (live && rl.aabb) {
#pragma unroll
      for (int k = 0; k < 3; ++k) live = live && p[k] >= rl.aabb[k] && p[k] <= rl.aabb[3 + k];
    }
  }
  __syncthreads();
  const bool staged = !mixed && f0 >= 0 && f0 < ps.F;      // block-uniform
  // cameras: kept iff any camera of the point's frame has it in view
  if (rl.cams) {
    if (staged) {
      for (int i = tid; i < (int)rl.C * LF_CAM; i += MC_THREADS) s_cam[i] = rl.cams[f0 * rl.C * LF_CAM + i];
      __syncthreads();
    }
    if (live) {
      bool seen = false;
      for (int64_t c = 0; c < rl.C && !seen; ++c) {
        const float* cam = staged ? s_cam + c * LF_CAM : rl.cams + (f * rl.C + c) * LF_CAM;
        const uint8_t* ign = rl.ignore ? rl.ignore + (f * rl.C + c) * rl.Hm * rl.Wm : nullptr;
        float u, v, d;
        seen = lf_in_view(cam, (int)((rl.models >> (2 * c)) & 3ull), p, rl.near_clip, ign, rl.Hm, rl.Wm, u, v, d);
      }
      live = seen;
    }
  }
  // boxes: kept iff inside no box of the point's frame
  if (rl.boxes) {
    if (staged) {
      int64_t lo = rl.box_off[f0], hi = rl.box_off[f0 + 1];
      lo = lo < 0 ? 0 : lo;
      hi = hi > rl.B ? rl.B : hi;
      for (int64_t b0 = lo; b0 < hi; b0 += LF_BOX_CHUNK) {
        const int nb = (int)(hi - b0 < LF_BOX_CHUNK ? hi - b0 : LF_BOX_CHUNK);
        __syncthreads();                            // the previous chunk (or the cameras) has been read
        for (int i = tid; i < nb * LF_BOX; i += MC_THREADS) s_box[i] = rl.boxes[b0 * LF_BOX + i];
        __syncthreads();
        for (int b = 0; b < nb && live; ++b) live = !lf_in_box(s_box + b * LF_BOX, p);
      }
    } else if (live) {
      int64_t lo = rl.box_off[f], hi = rl.box_off[f + 1];
      lo = lo < 0 ? 0 : lo;
      hi = hi > rl.B ? rl.B : hi;
      for (int64_t b = lo; b < hi && live; ++b) live = !lf_in_box(rl.boxes + b * LF_BOX, p);
    }
  }
  if (r < N) keep[r] = live ? 1 : 0;
  int tot;
  lr_block_rank(live ? 1 : 0, tot, wsum);
  if (tid == 0) cnt[blockIdx.x] = tot;
}

struct LfOut {
  float *rays_o, *rays_d, *ranges;
  int64_t *li, *fi, *keep_inds;
  float* pts_world;
};

__global__ void __launch_bounds__(MC_THREADS) k_lf_emit(const uint8_t* __restrict__ keep, const int32_t* __restrict__ off,
                                                      const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                      const float* __restrict__ ranges, int64_t N, LfPoses ps, LfOut out) {
  __shared__ int wsum[MC_THREADS / 64];
  const int64_t r = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  const int c = r < N && keep[r] ? 1 : 0;
  int tot;
  const int rank = lr_block_rank(c, tot, wsum);
  if (!c) return;
  const int64_t o = (int64_t)off[blockIdx.x] + rank;
  const float rg = ranges[r];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    out.rays_o[3 * o + k] = rays_o[3 * r + k];
    out.rays_d[3 * o + k] = rays_d[3 * r + k];
  }
  out.ranges[o] = rg;
  if (out.li) out.li[o] = ps.li[r];
  if (out.fi) out.fi[o] = ps.fi[r];
  if (out.keep_inds) out.keep_inds[o] = r;
  if (out.pts_world) {
    float p[3];
    int64_t f;
    lf_world_point(ps, rays_o, rays_d, rg, r, f, p);       // a kept point's indices are inside the tables
#pragma unroll
    for (int k = 0; k < 3; ++k) out.pts_world[3 * o + k] = p[k];
  }
}

// the dense projection of world points into C cameras: mask u8, u, v, d f32, all [C][N]
__global__ void __launch_bounds__(MC_THREADS) k_cam_project(const float* __restrict__ pts, int64_t N, const float* __restrict__ cams,
                                                          uint64_t models, int64_t C, float near_clip,
                                                          const uint8_t* __restrict__ ignore, int64_t Hm, int64_t Wm,
                                                          uint8_t* __restrict__ mask, float* __restrict__ u, float* __restrict__ v,
                                                          float* __restrict__ d) {
  __shared__ float s_cam[LF_MAX_CAMS * LF_CAM];
  for (int i = threadIdx.x; i < (int)C * LF_CAM; i += MC_THREADS) s_cam[i] = cams[i];
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  if (r >= N) return;
  const float p[3] = {pts[3 * r], pts[3 * r + 1], pts[3 * r + 2]};
  for (int64_t c = 0; c < C; ++c) {
    float uu, vv, dd;
    const bool in = lf_in_view(s_cam + c * LF_CAM, (int)((models >> (2 * c)) & 3ull), p, near_clip,
                               ignore ? ignore + c * Hm * Wm : nullptr, Hm, Wm, uu, vv, dd);
    mask[c * N + r] = in ? 1 : 0;
    u[c * N + r] = uu;
    v[c * N + r] = vv;
    d[c * N + r] = dd;
  }
}

// cam_models: HOST int32 [C], 0 pinhole / 1 opencv / 2 fisheye -> 2 bits each
static int lf_pack_models(const int32_t* cam_models, int64_t C, uint64_t& packed) {
  packed = 0;
  if (C < 0) return 2;
  if (C > LF_MAX_CAMS) return 62;
  if (C > 0 && !cam_models) return 62;
  for (int64_t c = 0; c < C; ++c) {
    if (cam_models[c] < 0 || cam_models[c] > 2) return 62;
    packed |= (uint64_t)cam_models[c] << (2 * c);
  }
  return 0;
}

extern "C" {

int nsim_lidar_filter_count(const float* rays_o, const float* rays_d, const float* ranges, const int64_t* li, const int64_t* fi,
                            int64_t N, const float* l2w, int64_t L, int64_t F, int filter_valid, const float* cams,
                            const int32_t* cam_models, int64_t C, float near_clip, const uint8_t* ignore, int64_t Hm, int64_t Wm,
                            const float* aabb, const float* boxes, const int32_t* box_offsets, int64_t B, uint8_t* keep,
                            int32_t* cnt, void* stream) {
  if (N < 0 || L < 0 || F < 0 || B < 0 || Hm < 0 || Wm < 0) return 2;
  if (N >= ((int64_t)1 << 31)) return 62;
  LfRule rl;
  const int rc = lf_pack_models(cam_models, C, rl.models);
  if (rc) return rc;
  if (N == 0) return 0;
  if (!keep || !cnt) return 4;
  if (!rays_o || !rays_d || !ranges || !l2w || L < 1 || F < 1) return 62;
  if ((C > 0 && !cams) || (ignore && (C == 0 || Hm < 1 || Wm < 1)) || (B > 0 && (!boxes || !box_offsets))) return 62;
  LfPoses ps = {l2w, li, fi, L, F};
  rl.filter_valid = filter_valid;
  rl.cams = C > 0 ? cams : nullptr;        // C = 0: no camera filter
  rl.C = C;
  rl.near_clip = near_clip;
  rl.ignore = ignore;
  rl.Hm = Hm;
  rl.Wm = Wm;
  rl.aabb = aabb;
  rl.boxes = B > 0 ? boxes : nullptr;      // B = 0: no box removes a point
  rl.box_off = box_offsets;
  rl.B = B;
  hipLaunchKernelGGL(k_lf_count, vg_blocks(N), dim3(MC_THREADS), 0, (hipStream_t)stream, rays_o, rays_d, ranges, N, ps, rl, keep, cnt);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_lidar_filter_emit(const uint8_t* keep, const int32_t* off, const float* rays_o, const float* rays_d, const float* ranges,
                           const int64_t* li, const int64_t* fi, int64_t N, const float* l2w, int64_t L, int64_t F,
                           float* out_rays_o, float* out_rays_d, float* out_ranges, int64_t* out_li, int64_t* out_fi,
                           int64_t* keep_inds, float* pts_world, void* stream) {
  if (N < 0 || L < 0 || F < 0) return 2;
  if (N >= ((int64_t)1 << 31)) return 62;
  if (N == 0) return 0;
  if (!out_rays_o || !out_rays_d || !out_ranges) return 4;
  if (!keep || !off || !rays_o || !rays_d || !ranges) return 62;
  if ((out_li && !li) || (out_fi && !fi) || (pts_world && (!l2w || L < 1 || F < 1))) return 62;
  LfPoses ps = {l2w, li, fi, L, F};
  LfOut out = {out_rays_o, out_rays_d, out_ranges, out_li, out_fi, keep_inds, pts_world};
  hipLaunchKernelGGL(k_lf_emit, vg_blocks(N), dim3(MC_THREADS), 0, (hipStream_t)stream, keep, off, rays_o, rays_d, ranges, N, ps, out);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_cam_project(const float* pts, int64_t N, const float* cams, const int32_t* cam_models, int64_t C, float near_clip,
                     const uint8_t* ignore, int64_t Hm, int64_t Wm, uint8_t* mask, float* u, float* v, float* d, void* stream) {
  if (N < 0 || Hm < 0 || Wm < 0) return 2;
  if (N >= ((int64_t)1 << 31)) return 62;
  uint64_t models;
  const int rc = lf_pack_models(cam_models, C, models);
  if (rc) return rc;
  if (N == 0 || C == 0) return 0;
  if (!mask || !u || !v || !d) return 4;
  if (!pts || !cams || (ignore && (Hm < 1 || Wm < 1))) return 62;
  hipLaunchKernelGGL(k_cam_project, vg_blocks(N), dim3(MC_THREADS), 0, (hipStream_t)stream, pts, N, cams, models, C, near_clip, ignore,
                     Hm, Wm, mask, u, v, d);
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
    case 51: return "nearest neighbours: sizes out of range (N, M < 2^31 - 1024, at most 65535 chunks, 1 <= max_cells < 2^30, target occupancy > 0)";
    case 52: return "sphere trace: fewer than 2^30 rays, max_march_iters >= 1 and min_step > 0";
    case 53: return "sphere trace: the runtime reports no resident workgroup for the kernel (CU count / occupancy query)";
    case 38: return "the close-range NeRF decoders take 1..16 LoTD levels (<= 32 input features)";
    case 39: return "n_appear must be 0 or 4";
    case 54: return "error map: n_images, h, w >= 1, n_images h w < 2^31 and a fixed frame below n_images";
    case 55: return "ssim: 1 <= window <= 11, stride >= 1, H W < 2^31, at least one window per image, the indexed form takes one image";
    case 56: return "occupancy grid: 1 <= subsample factor <= 4, resolutions >= 1, resolution * factor + 1 < 2^24 per axis, fewer than 2^31 voxels and lattice points per slab";
    case 57: return "visible grid: the grid edge is a power of two in 32 .. 1024 (octree depth 5 .. 10), fewer than 2^39 samples per call";
    case 58: return "street losses: unknown mode / type / function, lo > hi, more than 4 entropy terms or a source outside 0..2, 0 <= k < N < 2^32 for the order statistic, far / std > 0 where the function divides by it";
    case 59: return "segmentation z-buffer: at most 64 sources per call, candidate ordinals (ordinal_base + the call's candidates) below 2^32 - 1";
    case 60: return "lidar ray generation: thetas, phis and l2w are required, paired mode takes as many thetas as phis, fewer than 2^31 beams and azimuths and 2^39 rays";
    case 61: return "lidar returns: fewer than 2^31 rays per sweep; acc, depth, rays and offsets are required, and w2l / rgb / ids wherever their output is requested";
    case 62: return "lidar filter / camera projection: fewer than 2^31 points, at most 32 cameras per frame with model ids 0..2 (a host array), at least one frame and one lidar pose; rays, ranges and poses are required, and the camera / box / offset / source tables wherever their count or output asks for them";
    case 36: return "wide decoder: 0..10 embedding frequencies and at most 128 first-layer inputs (2 num_levels + 3 + 6 n_freq)";
    default: return code >= 1000 ? "HIP launch error (code - 1000 = hipError_t)" : "unknown error";
  }
}

}  // extern "C"
