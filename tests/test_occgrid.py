"""Occupancy grids (csrc/misc.hip ``nsim_occgrid_*``, neuralsim_amd/occgrid.py) against the per-voxel restatement
tests/occgrid_ref.py of ``code_single/tools/extract_occgrid.py``: the classifier on planted lattices, the bit-identical
coordinates, the callable and the model path, pruning by the model's occupancy grid, the .npz file, and the reference's own tool
on the shim."""
import math
import os
import subprocess
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import torch

import occgrid_ref as oref
import ref_glue
from util import make_params, model_from_params

ROOT = Path(__file__).resolve().parent.parent
REF = Path("/root/reference")
CFG = REF / "code_single/configs/object_centric/lotd_neus.dtu.230814.yaml"
TOOL = REF / "code_single/tools/extract_occgrid.py"


def _dev_lattice(a: np.ndarray, backend) -> torch.Tensor:
    """the lattice in a NaN-poisoned ``torch.empty`` buffer on the backend's device"""
    t = torch.empty(list(a.shape), dtype=torch.float32, device=backend)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
    return t


def _occ(a: np.ndarray, s: int, backend, **kw) -> np.ndarray:
    from neuralsim_amd import occgrid
    out = occgrid.occupancy_from_lattice(_dev_lattice(a, backend), s, **kw)
    assert out.dtype == torch.int32 and out.dim() == 2 and out.shape[1] == 3
    return out.cpu().numpy()


def _axes(res, s):
    ax = [np.linspace(-1.0, 1.0, r * s + 1, dtype=np.float32) for r in res]
    return np.meshgrid(*ax, indexing="ij")


def _fields(res, s):
    x, y, z = _axes(res, s)
    rng = np.random.default_rng(100 * s + res[0])
    out = {
        "sphere": np.sqrt(x * x + y * y + z * z) - 0.62,
        "two_spheres": np.minimum(np.sqrt((x + 0.3) ** 2 + y * y + (z - 0.1) ** 2) - 0.4,
                                  np.sqrt((x - 0.35) ** 2 + (y - 0.2) ** 2 + z * z) - 0.33),
        "noise": rng.standard_normal(x.shape),
        "all_positive": np.abs(rng.standard_normal(x.shape)) + 0.1,
        "all_negative": -np.abs(rng.standard_normal(x.shape)) - 0.1,
    }
    return {k: v.astype(np.float32) for k, v in out.items()}


def _planted(res, s, seed):
    """noise with 0.0, -0.0, +inf, -inf and NaN planted at lattice points shared by several voxels: voxel corners (index a
    multiple of s on all three axes: up to 8 owners), edges (two axes) and faces (one axis)"""
    rng = np.random.default_rng(seed)
    shape = [r * s + 1 for r in res]
    f = rng.standard_normal(shape).astype(np.float32)
    vals = [0.0, -0.0, np.inf, -np.inf, np.nan]
    for kind in ((1, 1, 1), (1, 1, 0), (0, 1, 1), (1, 0, 0), (0, 0, 1)):      # 1: on a voxel border along that axis
        for v in vals:
            j = []
            for a in range(3):
                i = int(rng.integers(0, res[a] + 1)) * s
                if not kind[a]:
                    i = min(i + (1 if s > 1 else 0), shape[a] - 1)
                j.append(i)
            f[tuple(j)] = v
    return f


RESOLUTIONS = [(40, 13, 9), (5, 3, 2), (1, 1, 1)]


# ------------------------------------------------------------------------------------------------ 1. classifier
@pytest.mark.parametrize("s", [1, 2, 3, 4])
@pytest.mark.parametrize("res", RESOLUTIONS)
def test_classifier_equals_per_voxel_restatement(backend, res, s):
    for name, f in _fields(res, s).items():
        got, want = _occ(f, s, backend), oref.classify(f, s)
        assert np.array_equal(got, want), (name, got.shape, want.shape)
        if name.startswith("all_"):
            assert got.shape == (0, 3)                       # the empty emission
    assert len(oref.classify(_fields(res, s)["noise"], s)) > 0
    for seed in range(4):
        f = _planted(res, s, seed)
        got, want = _occ(f, s, backend), oref.classify(f, s)
        assert np.array_equal(got, want), ("planted", seed)


@pytest.mark.parametrize("s", [1, 2])
def test_one_infinite_sample_empties_every_voxel_that_shares_it(backend, s):
    res = (5, 4, 3)
    x, y, z = np.meshgrid(*[np.arange(r * s + 1) for r in res], indexing="ij")
    f = np.where((x + y + z) % 2 == 0, 1.0, -1.0).astype(np.float32)       # both signs in every voxel
    assert len(_occ(f, s, backend)) == res[0] * res[1] * res[2]
    for val in (np.inf, -np.inf):
        g = f.copy()
        g[2 * s, 2 * s, 1 * s] = val                                      # a corner shared by 8 voxels
        got = {tuple(r) for r in _occ(g, s, backend).tolist()}
        gone = {(ix, iy, iz) for ix in (1, 2) for iy in (1, 2) for iz in (0, 1)}
        every = {(ix, iy, iz) for ix in range(res[0]) for iy in range(res[1]) for iz in range(res[2])}
        assert got == every - gone
    for val in (0.0, -0.0, np.nan):                                        # not positive, not infinite: still two signs
        g = f.copy()
        g[2 * s, 2 * s, 1 * s] = val
        assert len(_occ(g, s, backend)) == res[0] * res[1] * res[2]


def test_slab_independence(backend):
    res, s = (40, 13, 9), 2
    for f in (_fields(res, s)["two_spheres"], _planted(res, s, 11)):
        base = _occ(f, s, backend, slab=10 ** 6)
        assert len(base) > 0 and np.array_equal(base, oref.classify(f, s))
        for slab in (1, 4):
            assert np.array_equal(_occ(f, s, backend, slab=slab), base), slab


def test_state_marks_points_without_a_value(backend):
    """a point with a non-zero state has no sign: every voxel that owns it is empty, and its (poisoned) value is not read"""
    from neuralsim_amd import occgrid
    res, s = (5, 3, 2), 2
    f = _fields(res, s)["noise"]
    st = np.zeros(f.shape, dtype=np.uint8)
    st[4, 2, 2], st[7, 5, 1] = 2, 1
    g = f.copy()
    g[st != 0] = np.inf                        # the restatement: same as an infinite sample
    f[st != 0] = np.nan
    got = occgrid.occupancy_from_lattice(_dev_lattice(f, backend), s, state=torch.from_numpy(st).to(backend)).cpu().numpy()
    assert np.array_equal(got, oref.classify(g, s)) and len(got) < len(oref.classify(np.nan_to_num(f), s))


def test_refusals(backend):
    from neuralsim_amd import occgrid
    with pytest.raises(ValueError, match="subsample_factor"):
        occgrid.occupancy_from_lattice(torch.ones([6, 6, 6], device=backend), 5)
    with pytest.raises(ValueError, match="subsample_factor"):
        occgrid.extract_occupancy(lambda x: x[:, 0], aabb_world=[[0, 0, 0], [1, 1, 1]], occ_res=0.5, subsample_factor=0, device=backend)
    with pytest.raises(ValueError, match="res \\* s \\+ 1"):
        occgrid.occupancy_from_lattice(torch.ones([6, 5, 5], device=backend), 2)


def test_refuses_host_tensors():
    from neuralsim_amd import occgrid
    with pytest.raises(RuntimeError, match="no CPU path"):
        occgrid.occupancy_from_lattice(torch.ones([5, 5, 5]), 2)


# ------------------------------------------------------------------------------------------------ 2. coordinates
def _rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return torch.from_numpy(np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K).float()


def _frame_case():
    lo = torch.tensor([312.4, -208.7, 3.1])
    aabb_world = torch.stack([lo, lo + torch.tensor([7.3, 4.1, 2.9])])
    R = _rotation([0.3, -1.0, 0.55], 0.7)
    t = torch.tensor([315.9, -206.8, 4.6])
    scale = torch.tensor([1.7, 0.9, 1.2])
    obj_aabb = torch.tensor([[-1.9, -1.6, -1.1], [1.8, 2.1, 1.0]])
    return aabb_world, 0.37, R, t, scale, obj_aabb


@pytest.mark.parametrize("s", [2, 3])
def test_lattice_coordinates_are_bit_identical(backend, s):
    """the lattice-point kernel against the tool's expression evaluated with separate tensor operations on the same device --
    an FMA contraction or an approximate division in the kernel shows here.  The three products of the rotation are added left
    to right, ``(p0 + p1) + p2`` (``occgrid_ref.world_to_obj``): what ``sum(-1)`` does on the CPU, where the reference's tool is
    pinned (section 7); a device's ``sum(-1)`` may add them in another order (DESIGN section 7 records the MI355X's)."""
    from neuralsim_amd import occgrid
    aabb_world, occ_res, R, t, scale, obj_aabb = _frame_case()
    frame, res, a = occgrid.make_frame(aabb_world, occ_res, s, R, t, scale, obj_aabb)
    assert res == [19, 11, 7] and res == oref.resolution_of(aabb_world, occ_res).tolist()
    L = [r * s + 1 for r in res]
    x0, st0 = occgrid.lattice_points(frame, 0, 5, backend)
    x1, st1 = occgrid.lattice_points(frame, 5, L[0] - 5, backend)
    x, st = torch.cat([x0, x1]), torch.cat([st0, st1])
    assert x.shape == (L[0], L[1], L[2], 3) and st.shape == (L[0], L[1], L[2])
    # the shared-lattice form: index j at float(j // s) + sub[j % s]
    dev = backend
    aw, Rd, td, sd = aabb_world.to(dev), R.to(dev), t.to(dev), scale.to(dev)
    resolution = oref.resolution_of(aw, occ_res)
    sub = torch.arange(s + 1, device=dev, dtype=torch.float) / s
    c = [(torch.arange(n, device=dev) // s).float() + sub[torch.arange(n, device=dev) % s] for n in L]
    coords = torch.stack(torch.meshgrid(c, indexing="ij"), dim=-1)
    center, radius = (aw[1] + aw[0]) / 2.0, (aw[1] - aw[0]) / 2.0
    want = oref.world_to_obj(((coords / resolution) * 2 - 1) * radius + center, Rd, td, sd)
    assert torch.equal(x, want)
    b = obj_aabb.to(dev)
    inside = ((want >= b[0]) & (want <= b[1])).all(-1)
    assert torch.equal(st == 0, inside) and torch.equal(st == 1, ~inside)
    assert 0 < int(inside.sum()) < inside.numel()
    # the per-voxel form: both owners of a shared point see the kernel's bits
    block = [torch.arange(r, device=dev) for r in res]
    pv = oref.voxel_coords(block, resolution, s, aw, Rd, td, sd, dev)               # [X, Y, Z, (s + 1)^3, 3]
    k = torch.arange(s + 1, device=dev)
    jx = (block[0] * s)[:, None] + k
    jy = (block[1] * s)[:, None] + k
    jz = (block[2] * s)[:, None] + k
    shared = x[jx[:, None, None, :, None, None], jy[None, :, None, None, :, None], jz[None, None, :, None, None, :]]
    assert torch.equal(shared.reshape(pv.shape), pv)
    if dev.type == "cpu":
        # ... and what the tool itself runs on the shim: TransformMat4x4.forward(x, inv=True) / scale.vec_3()
        from nr3d_lib.models.attributes import TransformMat4x4
        M = torch.eye(4)
        M[:3, :3], M[:3, 3] = R, t
        tf = TransformMat4x4(M)
        xw = ((coords / resolution) * 2 - 1) * radius + center
        assert torch.equal(tf.forward(xw, inv=True) / scale, x)


# ------------------------------------------------------------------------------------------------ 3. callable path
def _analytic_sdf(x):
    sphere = torch.linalg.norm(x - torch.tensor([0.4, -0.2, 0.1], device=x.device), dim=-1) - 0.9
    q = (x - torch.tensor([-0.8, 0.6, -0.2], device=x.device)).abs() - torch.tensor([0.5, 0.7, 0.4], device=x.device)
    box = torch.linalg.norm(q.clamp_min(0.0), dim=-1) + q.max(dim=-1).values.clamp_max(0.0)
    return torch.minimum(sphere, box)


def test_callable_path_equals_per_voxel_algorithm(backend):
    from neuralsim_amd import occgrid
    aabb_world, occ_res, R, t, scale, obj_aabb = _frame_case()
    s = 2
    kw = dict(aabb_world=aabb_world, occ_res=occ_res, subsample_factor=s, rotation=R, translation=t, scale=scale, device=backend)
    calls = []

    def counted(x):
        calls.append(x.shape[0])
        return _analytic_sdf(x)
    free = occgrid.extract_occupancy(counted, chunk=700, slab=3, **kw)
    n_ref = [0]
    ref, rl = oref.extract_per_voxel(_analytic_sdf, aabb_world=aabb_world, occ_res=occ_res, s=s, R=R, t=t, scale=scale, dev=backend,
                                     counter=n_ref)
    assert free["resolution"] == rl == [19, 11, 7]                                   # truncation: 7.3 / 0.37 = 19.7 -> 19
    assert np.array_equal(free["coord_min"], aabb_world[0].numpy())
    got = free["occ_corners"].cpu().numpy()
    assert len(ref) > 50 and np.array_equal(got, oref.sort_rows(ref))               # every voxel, order included
    L = [r * s + 1 for r in rl]
    assert free["stats"]["n_lattice"] == L[0] * L[1] * L[2] == free["stats"]["n_queried"] == sum(calls)
    assert n_ref[0] == 27 * rl[0] * rl[1] * rl[2] and max(calls) <= 700
    # independent of slab and chunk
    for slab, chunk in ((1, 10 ** 6), (None, 4096)):
        again = occgrid.extract_occupancy(_analytic_sdf, chunk=chunk, slab=slab, **kw)
        assert torch.equal(again["occ_corners"], free["occ_corners"])
    # points that leave the object box are not queried, and their voxels are dropped
    seen = []

    def watched(x):
        seen.append(x.detach().cpu())
        return _analytic_sdf(x)
    boxed = occgrid.extract_occupancy(watched, obj_aabb=obj_aabb, chunk=5000, **kw)
    refb, _ = oref.extract_per_voxel(_analytic_sdf, aabb_world=aabb_world, occ_res=occ_res, s=s, R=R, t=t, scale=scale,
                                     obj_aabb=obj_aabb, dev=backend)
    gb = boxed["occ_corners"].cpu().numpy()
    assert np.array_equal(gb, oref.sort_rows(refb)) and 0 < len(gb) < len(got)
    pts = torch.cat(seen)
    assert bool(((pts >= obj_aabb[0]) & (pts <= obj_aabb[1])).all())
    st = boxed["stats"]
    assert st["n_queried"] == pts.shape[0] and st["n_out_of_box"] == st["n_lattice"] - st["n_queried"] > 0 and st["n_pruned"] == 0


# ------------------------------------------------------------------------------------------------ 4. model path
_RADIUS = 0.5                 # oracle.field.make_field_params(radius_init=0.5)


def _sphere_model(backend):
    return model_from_params(make_params(sphere=True), backend)


def _model_query(m):
    grid16, wpack = m._shadow()

    def q(x):
        return m._sdf_query(grid16, wpack, x.contiguous(), None, None, None, None, x.shape[0], m.device)
    return q


def _model_ref(m, occ_res, s, backend):
    from neuralsim_amd import occgrid
    with torch.no_grad():
        aw = occgrid.model_world_aabb(m).cpu()
        return oref.extract_per_voxel(_model_query(m), aabb_world=aw, occ_res=occ_res, s=s, R=torch.eye(3), t=torch.zeros(3),
                                      scale=torch.ones(3), obj_aabb=m.space.aabb.cpu(), dev=backend)


def test_model_path_equals_per_voxel_algorithm(backend):
    """the shared lattice through the model's query against 27 queries per voxel in 64^3 blocks through the same query: equal
    sets, no tolerance (the query is per-point arithmetic: the batch a point travels in does not change its value)"""
    from neuralsim_amd import occgrid
    m = _sphere_model(backend)
    n = 24 if backend.type == "cpu" else 48
    occ_res = 2.0 / n - 1e-4
    out = occgrid.extract_occupancy_from_model(m, occ_res=occ_res, slab=7)
    ref, rl = _model_ref(m, occ_res, 2, backend)
    got = out["occ_corners"].cpu().numpy()
    assert out["resolution"] == rl == [n, n, n]
    diff = len(set(map(tuple, got.tolist())) ^ set(map(tuple, ref.tolist())))
    print(f"model path: {len(got)} voxels, {len(ref)} per-voxel, symmetric difference {diff}")
    assert len(ref) > 100 and np.array_equal(got, oref.sort_rows(ref))
    assert out["stats"]["n_queried"] == out["stats"]["n_lattice"] == (2 * n + 1) ** 3
    # a closed shell around the sphere: every centre within one voxel diagonal of radius r, and a voxel along every axis ray
    edge = 2.0 / n
    ctr = -1.0 + (got.astype(np.float64) + 0.5) * edge
    assert np.abs(np.linalg.norm(ctr, axis=-1) - _RADIUS).max() <= math.sqrt(3.0) * edge
    mid = n // 2
    for ax in range(3):
        o = [a for a in range(3) if a != ax]
        on = got[(np.abs(got[:, o[0]] - mid + 0.5) <= 0.5) & (np.abs(got[:, o[1]] - mid + 0.5) <= 0.5)]
        assert (on[:, ax] < mid).any() and (on[:, ax] >= mid).any()
    # the whole grid in one slab, and another chunking of the queries
    again = occgrid.extract_occupancy_from_model(m, occ_res=occ_res, slab=10 ** 6, chunk=50000)
    assert torch.equal(again["occ_corners"], out["occ_corners"])


def _check_forward_in_obj(m, backend):
    g = torch.Generator().manual_seed(5)
    x = (torch.rand([400, 3], generator=g) * 2.6 - 1.3).to(backend)
    a = m.space.aabb
    inside = ((x >= a[0]) & (x <= a[1])).all(-1)
    assert 0 < int(inside.sum()) < 400
    r = m.implicit_surface.forward_in_obj(x, invalid_sdf=np.inf, return_h=False, with_normal=False)
    assert set(r) == {"sdf"} and r["sdf"].shape == (400,) and not r["sdf"].requires_grad
    assert bool(torch.isposinf(r["sdf"][~inside]).all()) and bool(torch.isfinite(r["sdf"][inside]).all())
    want = m.forward_sdf(x[inside])["sdf"].detach()
    # the no-grad query and the with-grad forward are two kernels over the same f32 weights: the bound of the lattice test of
    # tests/test_mesh.py (2e-5) on |sdf| < 2
    assert (r["sdf"][inside] - want).abs().max() <= 2e-5
    r2 = m.forward_in_obj(x.view(20, 20, 3), invalid_sdf=-7.0, with_normal=True)
    assert r2["sdf"].shape == (20, 20) and r2["nablas"].shape == (20, 20, 3)
    assert bool((r2["sdf"].view(-1)[~inside] == -7.0).all()) and torch.equal(r2["sdf"].view(-1)[inside], r["sdf"][inside])
    nb = m.forward_sdf_nablas(x[inside], nablas_has_grad=False)["nablas"].detach()
    assert torch.equal(r2["nablas"].view(-1, 3)[inside], nb) and bool((r2["nablas"].view(-1, 3)[~inside] == 0).all())
    with pytest.raises(NotImplementedError, match="return_h"):
        m.forward_in_obj(x, return_h=True)


def test_forward_in_obj(backend):
    _check_forward_in_obj(_sphere_model(backend), backend)


def test_permuto_model(backend):
    from neuralsim_amd import occgrid
    from neuralsim_amd.fields.permuto_neus import PermutoNeuSModel
    cfg = dict(type="multi_res", n_levels=6, n_feats=2, log2_hashmap_size=11, coarsest_res=2.0, finest_res=24.0,
               apply_random_shifts_per_level=True, seed=5)
    m = PermutoNeuSModel(permuto_auto_compute_cfg=cfg, sdf_D=1, precision="f32", param_bound=1.0, seed=9).to(backend)
    _check_forward_in_obj(m, backend)
    occ_res = 2.0 / 10 - 1e-4
    out = occgrid.extract_occupancy_from_model(m, occ_res=occ_res, subsample_factor=1)
    ref, rl = _model_ref(m, occ_res, 1, backend)
    assert out["resolution"] == rl == [10, 10, 10]
    assert len(ref) > 0 and np.array_equal(out["occ_corners"].cpu().numpy(), oref.sort_rows(ref))


# ------------------------------------------------------------------------------------------------ 5. pruning
def _sample_cells(m, out, s, backend):
    """cells of the model's occupancy grid that contain a sample point of an occupied voxel of ``out``"""
    from neuralsim_amd import occgrid
    frame, res, _ = occgrid.make_frame(occgrid.model_world_aabb(m), out["occ_res"], s, obj_aabb=m.space.aabb)
    x, _ = occgrid.lattice_points(frame, 0, res[0] * s + 1, backend)
    v = out["occ_corners"].long()
    k = torch.arange(s + 1, device=backend)
    j = [(v[:, a] * s)[:, None] + k for a in range(3)]
    pts = x[j[0][:, :, None, None], j[1][:, None, :, None], j[2][:, None, None, :]].reshape(-1, 3)
    return occgrid.accel_cells_of(m.accel, pts)


def _set_cells(m, cells):
    with torch.no_grad():
        m.accel.occ_val.zero_()
        m.accel.occ_val[cells] = 1.0
    m.accel.pack_bits()


def test_prune_by_the_models_occupancy_grid(backend):
    from neuralsim_amd import occgrid
    m = _sphere_model(backend)
    n = 24 if backend.type == "cpu" else 48
    occ_res = 2.0 / n - 1e-4
    full = occgrid.extract_occupancy_from_model(m, occ_res=occ_res)
    assert len(full["occ_corners"]) > 100
    # every cell occupied: nothing is pruned
    m.accel.set_all_occupied()
    a = occgrid.extract_occupancy_from_model(m, occ_res=occ_res, prune="accel")
    assert torch.equal(a["occ_corners"], full["occ_corners"])
    assert a["stats"]["n_queried"] == a["stats"]["n_lattice"] - a["stats"]["n_out_of_box"] and a["stats"]["n_pruned"] == 0
    # the minimal grid: exactly the cells that contain a sample point of an occupied voxel
    _set_cells(m, _sample_cells(m, full, 2, backend))
    b = occgrid.extract_occupancy_from_model(m, occ_res=occ_res, prune="accel", slab=5)
    assert torch.equal(b["occ_corners"], full["occ_corners"])
    assert 0 < b["stats"]["n_queried"] < b["stats"]["n_lattice"] and b["stats"]["n_pruned"] > 0
    assert b["stats"]["n_queried"] + b["stats"]["n_pruned"] + b["stats"]["n_out_of_box"] == b["stats"]["n_lattice"]


def test_prune_one_cell_removed_gives_a_strict_subset(backend):
    """The rule dilates by one cell, so a removed cell deactivates a point only if its 26 neighbours are empty too.  On a lattice
    whose points are more than two cells apart (24^3 voxels, s = 1: 2.67 cells of the model's 64^3 grid) the cells of the minimal
    grid are pairwise non-adjacent: removing one deactivates exactly the sample points it contains."""
    from neuralsim_amd import occgrid
    m = _sphere_model(backend)
    assert list(m.accel.resolution) == [64, 64, 64]
    occ_res = 2.0 / 24 - 1e-4
    full = occgrid.extract_occupancy_from_model(m, occ_res=occ_res, subsample_factor=1)
    cells = torch.unique(_sample_cells(m, full, 1, backend))
    _set_cells(m, cells)
    same = occgrid.extract_occupancy_from_model(m, occ_res=occ_res, subsample_factor=1, prune="accel")
    assert torch.equal(same["occ_corners"], full["occ_corners"]) and same["stats"]["n_queried"] < same["stats"]["n_lattice"]
    _set_cells(m, cells[cells != cells[len(cells) // 2]])
    less = occgrid.extract_occupancy_from_model(m, occ_res=occ_res, subsample_factor=1, prune="accel")
    f = set(map(tuple, full["occ_corners"].cpu().tolist()))
    l = set(map(tuple, less["occ_corners"].cpu().tolist()))
    assert l < f                                                # strict subset: nothing the unpruned run lacks
    assert less["stats"]["n_queried"] == same["stats"]["n_queried"] - 1


def test_prune_needs_an_occupancy_grid():
    from neuralsim_amd import occgrid
    with pytest.raises(ValueError, match="model.accel"):
        occgrid.extract_occupancy_from_model(types.SimpleNamespace(device=torch.device("cpu")), occ_res=0.1, prune="accel")
    with pytest.raises(ValueError, match="prune"):
        occgrid.extract_occupancy_from_model(types.SimpleNamespace(), occ_res=0.1, prune="grid")


# ------------------------------------------------------------------------------------------------ 6. npz
def test_npz_round_trip(tmp_path):
    from neuralsim_amd import occgrid
    occ = torch.tensor([[0, 1, 2], [3, 0, 1], [299, 31, 7]], dtype=torch.int32)
    res = dict(occ_corners=occ, resolution=[300, 32, 8], coord_min=np.array([1.5, -2.0, 0.25], dtype=np.float32), occ_res=0.1,
               stats={})
    path = tmp_path / "g.npz"
    occgrid.write_occgrid_npz(str(path), res, coord_offset=np.array([10.0, 20.0, 30.0]), meta=dict(scene_id="s0", start_frame=3, num_frames=9))
    d = np.load(str(path), allow_pickle=True)
    assert sorted(d.files) == sorted(["occ_corners", "sidelength", "occ_res", "coord_min", "coord_offset", "meta"])
    assert d["occ_corners"].dtype == np.int16 and np.array_equal(d["occ_corners"], occ.numpy())
    assert d["sidelength"].tolist() == [300, 32, 8] and float(d["occ_res"]) == 0.1
    assert d["coord_min"].dtype == np.float32 and np.array_equal(d["coord_min"], res["coord_min"])
    assert d["coord_offset"].tolist() == [10.0, 20.0, 30.0] and d["meta"].item()["num_frames"] == 9
    with pytest.raises(ValueError, match="32767"):
        occgrid.write_occgrid_npz(str(tmp_path / "h.npz"), dict(res, resolution=[32768, 2, 2]))


def test_shim_voxel_verts():
    from nr3d_lib.models.grid_encodings.utils import voxel_verts
    v = voxel_verts(_0=-1., _1=1.)
    assert v.shape == (8, 3) and len({tuple(r) for r in v.tolist()}) == 8
    assert v.min(0).values.tolist() == [-1.0] * 3 and v.max(0).values.tolist() == [1.0] * 3


# ------------------------------------------------------------------------------------------------ 7. reference tool
needs_reference = ref_glue.needs_reference(ref_glue.readable(CFG) and ref_glue.readable(TOOL),
                                           reason="executes the reference's own sources, which only the authoring machine has (emulator backend)")


@needs_reference
def test_reference_extract_occgrid_tool_runs_unchanged(backend, tmp_path):
    """``code_single/tools/extract_occgrid.py``, source unchanged, on an experiment the reference's trainer wrote on this
    package; the same checkpoint through ``extract_occupancy_from_model`` gives the same voxels."""
    import importlib
    from neuralsim_amd import occgrid
    from nr3d_lib.checkpoint import sorted_ckpts
    from nr3d_lib.config import load_config
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    from test_reference_train import _run
    exp = tmp_path / "exp"
    r = _run(exp, ["--num_iters=4", "--training.i_val=-1", "--training.i_log=4"])
    assert r.returncode == 0 and "Everything done." in r.stdout, (r.stdout + r.stderr)[-3000:]
    c = load_config(str(exp / "config.yaml"))
    state = torch.load(sorted_ckpts(str(exp / "ckpts"))[-1], map_location="cpu", weights_only=False)
    key = next(k for k in state["asset_bank"] if k.startswith("LoTDNeuSObj#Main"))
    with ref_glue.reference_model_wrapper_modules():
        single = importlib.import_module("app.models.single")
        model = single.LoTDNeuSObj(**c.assetbank_cfg.Main.model_params.to_dict(), device=backend)
        loaded = model.load_state_dict(state["asset_bank"][key], strict=False)
        assert not [k for k in loaded.missing_keys if "encoding" in k or "sdf_" in k], loaded.missing_keys
    model.to(backend)
    ext = (model.space.aabb[1] - model.space.aabb[0]).min().item()
    occ_res = round(ext / 12.3, 4)
    env = dict(os.environ, PYTHONWARNINGS="ignore")
    cmd = [sys.executable, str(ROOT / "tools" / "run_reference_train.py"), "--emulate", "--script",
           "code_single/tools/extract_occgrid.py", "--resume_dir", str(exp), "--occ_res", str(occ_res)]
    rr = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=str(ROOT))
    assert rr.returncode == 0, (rr.stdout + rr.stderr)[-3000:]
    files = list((exp / "occgrid").glob("*.npz"))
    assert len(files) == 1, list((exp / "occgrid").iterdir())
    d = np.load(str(files[0]), allow_pickle=True)
    assert sorted(d.files) == sorted(["occ_corners", "sidelength", "occ_res", "coord_min", "coord_offset", "meta"])
    assert d["occ_corners"].dtype == np.int16 and min(d["sidelength"].tolist()) == 12
    out = occgrid.extract_occupancy_from_model(model, occ_res=occ_res, subsample_factor=2)
    assert out["resolution"] == d["sidelength"].tolist() and np.array_equal(out["coord_min"], d["coord_min"])
    assert len(d["occ_corners"]) > 0
    assert np.array_equal(out["occ_corners"].cpu().numpy(), oref.sort_rows(d["occ_corners"]))
