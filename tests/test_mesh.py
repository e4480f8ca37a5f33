"""Marching cubes (csrc/misc.hip ``nsim_mc_*``, neuralsim_amd/mesh.py) against the numpy restatement tests/mesh_ref.py, the
topology / geometry of its meshes, the model path against the oracle, the PLY writer, and the reference's own
``code_single/tools/extract_mesh.py`` on the shim."""
import math
import os
import subprocess
import sys
from collections import Counter
from pathlib import Path

import numpy as np
import pytest
import torch

import mesh_ref
import ref_glue
from oracle import field as ofield
from util import SMALL_RES, make_params, model_from_params

ROOT = Path(__file__).resolve().parent.parent
REF = Path("/root/reference")
CFG = REF / "code_single/configs/object_centric/lotd_neus.dtu.230814.yaml"


def _mc(lat, bmin, h, level=0.0, **kw):
    from neuralsim_amd import mesh
    v, f, n = mesh.marching_cubes(lat, bmin, h, level, **kw)
    return v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy()


def _grid(n, lo=-1.0, hi=1.0, shape=None):
    nx, ny, nz = shape if shape is not None else (n, n, n)
    h = (hi - lo) / (n - 1)
    ax = [np.float32(lo) + np.float32(h) * np.arange(m, dtype=np.float32) for m in (nx, ny, nz)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return x, y, z, h


def _sphere(x, y, z, r=0.6, c=(0.0, 0.0, 0.0)):
    return np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r


def _torus(x, y, z, R=0.55, r=0.22):
    return np.sqrt((np.sqrt(x * x + y * y) - R) ** 2 + z * z) - r


FIELDS = {
    "sphere": lambda x, y, z: _sphere(x, y, z),
    "torus": lambda x, y, z: _torus(x, y, z),
    "two_spheres": lambda x, y, z: np.minimum(_sphere(x, y, z, 0.45, (-0.25, 0.0, 0.1)), _sphere(x, y, z, 0.4, (0.3, 0.1, -0.1))),
}


def _euler(V, F):
    e = np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), axis=1)
    return V - len(np.unique(e, axis=0)) + len(F)


def _volume(v, F):
    a, b, c = (v[F[:, q]].astype(np.float64) for q in range(3))
    return float((a * np.cross(b, c)).sum() / 6.0)


def _assert_closed(F):
    """every undirected edge used exactly twice, once in each direction"""
    d = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]])
    cnt = Counter(map(tuple, d.tolist()))
    assert all(c == 1 for c in cnt.values()), "a directed edge is used twice"
    assert all((b, a) in cnt for (a, b) in cnt), "an edge is used by one triangle only"


def _assert_parity(f, bmin, h, level=0.0, **kw):
    v, F, n = _mc(f, bmin, h, level, **kw)
    rv, rF, rn = mesh_ref.marching_cubes(f.cpu().numpy() if isinstance(f, torch.Tensor) else f, bmin, h, level)
    assert v.shape == rv.shape and F.shape == rF.shape, (v.shape, rv.shape, F.shape, rF.shape)
    assert (F == rF).all()
    assert np.abs(v - rv).max(initial=0.0) <= 1e-6
    assert np.abs(n - rn).max(initial=0.0) <= 1e-5
    return v, F, n


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres"])
def test_parity_with_restatement(backend, name):
    n = 40 if backend.type == "cpu" else 128
    x, y, z, h = _grid(n)
    f = FIELDS[name](x, y, z).astype(np.float32)
    v, F, _ = _assert_parity(torch.from_numpy(f).to(backend), [-1.0, -1.0, -1.0], h)
    assert len(F) > 100


def test_parity_plane_through_lattice_points(backend):
    """corners exactly == level: plane z = const through a lattice plane, and a tilted plane on integer values"""
    n = 24 if backend.type == "cpu" else 96
    k = np.arange(n, dtype=np.float32)
    z, y, x = np.meshgrid(k, k, k, indexing="ij")
    for f in ((z - 10.0).astype(np.float32), (x + y - z - 7.0).astype(np.float32)):
        v, F, _ = _assert_parity(torch.from_numpy(np.ascontiguousarray(f)).to(backend), [0.0, 0.0, 0.0], 1.0)
        assert len(F) > 0


def test_level_and_cuboid_grid(backend):
    x, y, z, h = _grid(30, shape=(23, 30, 17))
    f = _sphere(x, y, z * 1.5, 0.5).astype(np.float32)
    _assert_parity(torch.from_numpy(f).to(backend), [-1.0, -1.0, -1.0], h, level=0.07)


# ------------------------------------------------------------------------------------------------ 2. slab independence
def test_slab_independence(backend):
    n = 33 if backend.type == "cpu" else 100
    x, y, z, h = _grid(n)
    f = torch.from_numpy(FIELDS["two_spheres"](x, y, z).astype(np.float32)).to(backend)
    base = _mc(f, [-1.0, -1.0, -1.0], h, slab=10 ** 6)
    for slab in (1, 3, 7):
        v, F, nrm = _mc(f, [-1.0, -1.0, -1.0], h, slab=slab)
        assert np.array_equal(v, base[0]) and np.array_equal(F, base[1]) and np.array_equal(nrm, base[2]), slab
    # a callable that fills slab planes gives the same mesh as the whole lattice
    calls = []

    def fill(k0, m, out):
        calls.append((k0, m))
        out.copy_(f[k0:k0 + m])
    v, F, nrm = _mc(fill, [-1.0, -1.0, -1.0], h, shape=(n, n, n), slab=5, device=backend)
    assert np.array_equal(v, base[0]) and np.array_equal(F, base[1]) and np.array_equal(nrm, base[2])
    assert sum(m for _, m in calls) < n + 3 * len(calls)          # every plane is asked for about once


# ------------------------------------------------------------------------------------------------ 3. topology / geometry
def test_noise_fields_are_crack_free(backend):
    rng = np.random.default_rng(7)
    for s in range(6 if backend.type == "cpu" else 20):
        shape = (int(rng.integers(6, 16)), int(rng.integers(6, 16)), int(rng.integers(6, 16)))
        f = rng.uniform(-1.0, 1.0, shape).astype(np.float32)
        f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = 1.0, 1.0, 1.0, 1.0, 1.0, 1.0
        v, F, _ = _mc(torch.from_numpy(f).to(backend), [0.0, 0.0, 0.0], 1.0, slab=int(rng.integers(1, 5)))
        assert len(F) > 0
        _assert_closed(F)


def test_sphere_euler_volume_orientation(backend):
    n = 96
    r = 0.7
    x, y, z, h = _grid(n)
    v, F, nrm = _mc(torch.from_numpy(_sphere(x, y, z, r).astype(np.float32)).to(backend), [-1.0, -1.0, -1.0], h)
    _assert_closed(F)
    assert _euler(len(v), F) == 2
    vol = _volume(v, F)
    assert vol > 0 and abs(vol - 4.0 / 3.0 * math.pi * r ** 3) < 0.01 * 4.0 / 3.0 * math.pi * r ** 3, vol
    # face normals point outwards (towards increasing SDF), and so do the vertex normals
    a, b, c = (v[F[:, q]] for q in range(3))
    fn = np.cross(b - a, c - a)
    assert ((fn * (a + b + c)).sum(-1) > 0).mean() > 0.999
    assert ((nrm * v).sum(-1) > 0.99 * np.linalg.norm(v, axis=-1)).all()
    assert np.abs(np.linalg.norm(v, axis=-1) - r).max() < h * h


def test_torus_euler_zero(backend):
    x, y, z, h = _grid(48)
    v, F, _ = _mc(torch.from_numpy(_torus(x, y, z).astype(np.float32)).to(backend), [-1.0, -1.0, -1.0], h, slab=9)
    _assert_closed(F)
    assert _euler(len(v), F) == 0


def test_vertices_lie_on_their_owner_edges(backend):
    x, y, z, h = _grid(28)
    f = FIELDS["two_spheres"](x, y, z).astype(np.float32)
    v, F, _ = _mc(torch.from_numpy(f).to(backend), [-1.0, -1.0, -1.0], h)
    q = (v.astype(np.float64) + 1.0) / h
    on = np.abs(q - np.round(q)) < 1e-3
    assert (on.sum(-1) >= 2).all()
    for vi in range(0, len(v), 7):      # the two ends of the owner edge straddle the level
        ax = int(np.argmin(on[vi])) if on[vi].sum() == 2 else 0
        i0 = np.floor(q[vi] + np.where(on[vi], 0.5, 0.0)).astype(int)
        i1 = i0.copy()
        i1[ax] += 1
        a, b = f[i0[2], i0[1], i0[0]], f[i1[2], i1[1], i1[0]]
        assert (a < 0) != (b < 0) or a == 0 or b == 0, (vi, a, b)


# ------------------------------------------------------------------------------------------------ 4. edge cases
def test_no_crossing_gives_empty_mesh(backend):
    f = torch.ones([9, 8, 7], device=backend)
    v, F, n = _mc(f, [0.0, 0.0, 0.0], 1.0)
    assert v.shape == (0, 3) and F.shape == (0, 3) and n.shape == (0, 3)
    v, F, n = _mc(torch.ones([1, 5, 5], device=backend), [0.0, 0.0, 0.0], 1.0)
    assert v.shape == (0, 3) and F.shape == (0, 3)


def test_nan_corners_emit_nothing(backend):
    x, y, z, h = _grid(26)
    f = _sphere(x, y, z).astype(np.float32)
    clean = _mc(torch.from_numpy(f).to(backend), [-1.0, -1.0, -1.0], h)
    f[5:9, 10:13, 3:20] = np.nan
    f[20, 20, 20] = np.inf
    v, F, n = _assert_parity(torch.from_numpy(f).to(backend), [-1.0, -1.0, -1.0], h, slab=4)
    assert np.isfinite(v).all() and np.isfinite(n).all()
    assert 0 < len(F) < len(clean[1]) and F.max() < len(v)
    # the mesh away from the poisoned region is untouched
    far = lambda vv: vv[(vv[:, 2] > 0.3)]
    assert np.array_equal(np.sort(far(v), axis=0), np.sort(far(clean[0]), axis=0))


def test_cuboid_box_per_axis_counts(backend):
    from neuralsim_amd import mesh
    bmin, bmax = [0.0, -1.0, 0.5], [1.0, 1.0, 3.5]
    h, shape = mesh.lattice_shape(bmin, bmax, 11)
    assert abs(h - 0.1) < 1e-12 and shape == (11, 21, 31)
    seen = []

    def sdf(x):
        seen.append(x.detach().cpu())
        return torch.linalg.norm(x - torch.tensor([0.5, 0.0, 2.0], device=x.device), dim=-1) - 0.4
    out = mesh.extract_mesh(sdf, bmin=bmin, bmax=bmax, N=11, chunk=500, show_progress=False, device=backend)
    pts = torch.cat(seen)
    assert pts.shape[0] == 11 * 21 * 31 and max(s.shape[0] for s in seen) <= 500
    assert torch.allclose(pts.min(0).values, torch.tensor(bmin)) and torch.allclose(pts.max(0).values, torch.tensor(bmax), atol=1e-5)
    v, F = out["verts"], out["faces"]
    _assert_closed(F)
    assert _euler(len(v), F) == 2 and (v.min(0) > np.array(bmin)).all() and (v.max(0) < np.array(bmax)).all()


def test_refuses_host_tensors():
    from neuralsim_amd import mesh
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.marching_cubes(torch.ones([4, 4, 4]), [0.0, 0.0, 0.0], 1.0)


# ------------------------------------------------------------------------------------------------ 5. model path
def test_model_path_against_oracle(backend):
    from neuralsim_amd import mesh
    p = make_params(sphere=True)
    m = model_from_params(p, backend)
    N = 24 if backend.type == "cpu" else 64
    fill, h, shape, bmin = mesh.model_lattice_fill(m, N)
    nx, ny, nz = shape
    lat = torch.empty([nz, ny, nx], device=backend)
    fill(0, nz, lat)
    pts = mesh._lattice_points(bmin, h, nx, ny, 0, nz, torch.device("cpu")).reshape(-1, 3)
    with torch.no_grad():
        ref = ofield.forward_sdf(pts, p).reshape(nz, ny, nx)
    assert (lat.cpu() - ref).abs().max() <= 2e-5
    out = mesh.extract_mesh_from_model(m, N, include_color=True, slab=5)
    v, F = out["verts"], out["faces"]
    assert len(F) > 0
    _assert_closed(F)
    assert _euler(len(v), F) == 2
    # the same mesh as marching cubes on the oracle's lattice (up to the query's rounding at near-zero corners)
    assert abs(len(v) - len(mesh_ref.marching_cubes(ref.numpy(), bmin, h)[0])) <= max(2, len(v) // 200)
    with torch.no_grad():
        sv = ofield.forward_sdf(torch.from_numpy(v), p)
    assert sv.abs().max() < h * h, (float(sv.abs().max()), h * h)          # linear interpolation along the edges: O(h^2)
    # colours: model.forward at the vertices, seen along -normals, against the oracle's field forward
    vv = torch.from_numpy(v)
    d = -torch.from_numpy(out["normals"])
    _, _, rgb_ref = ofield.forward_field(vv, d, torch.zeros([len(v), 4]), p)
    col_ref = (rgb_ref.detach().clamp(0, 1) * 255.0).round()
    assert (torch.from_numpy(out["colors"]).float() - col_ref).abs().max() <= 1.0
    with torch.no_grad():
        got = m.forward(vv.to(backend), d.to(backend), with_rgb=True, with_normal=True)
    assert (got["rgb"].cpu() - rgb_ref.detach()).abs().max() < 1e-4
    assert (got["sdf"].cpu() - sv).abs().max() < 1e-4 and got["nablas"].shape == (len(v), 3)


def test_input_normalized_mapping(backend):
    from neuralsim_amd.fields.neus import LoTDNeuSModel
    aabb = torch.tensor([[-2.0, -1.0, 0.0], [2.0, 1.5, 3.0]])
    m = LoTDNeuSModel(lod_res=SMALL_RES, log2_hashmap_size=12, aabb=aabb, precision="f32").to(backend)
    with torch.no_grad():
        n_p = m.encoding.flattened_params.numel()
        m.encoding.flattened_params.copy_((torch.rand(n_p, generator=torch.Generator().manual_seed(3)) * 0.6 - 0.3).to(backend))
    g = torch.Generator().manual_seed(4)
    xn = (torch.rand(300, 3, generator=g) * 2 - 1).to(backend)
    x = aabb[0].to(backend) + (xn + 1) * 0.5 * (aabb[1] - aabb[0]).to(backend)
    a = m.forward_sdf(xn, input_normalized=True)["sdf"]
    b = m.forward_sdf(x, input_normalized=False)["sdf"]
    assert (a - b).abs().max() < 1e-5 and (b - m.forward_sdf(x)["sdf"]).abs().max() == 0
    an = m.forward_sdf_nablas(xn, input_normalized=True)["nablas"]
    bn = m.forward_sdf_nablas(x)["nablas"]
    assert (an - bn).abs().max() < 1e-3 * (1 + bn.abs().max())
    v = torch.nn.functional.normalize(torch.randn(300, 3, generator=g), dim=-1).to(backend)
    fa = m.forward(xn, v, input_normalized=True)
    fb = m.forward(x, v)
    assert set(fa) == {"sdf", "rgb"} and (fa["rgb"] - fb["rgb"]).abs().max() < 1e-5
    assert (fb["sdf"] - b).abs().max() < 1e-5


# ------------------------------------------------------------------------------------------------ 6. PLY
def _read_ply(path):
    data = Path(path).read_bytes()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    nv = int(next(l for l in head if l.startswith("element vertex")).split()[-1])
    nf = int(next(l for l in head if l.startswith("element face")).split()[-1])
    props = [l.split()[-1] for l in head if l.startswith("property") and "list" not in l]
    assert props[:3] == ["x", "y", "z"]
    color = props[3:] == ["red", "green", "blue"]
    assert "property list uchar int vertex_indices" in head
    vd = np.dtype([("xyz", "<f4", (3,))] + ([("rgb", "u1", (3,))] if color else []))
    verts = np.frombuffer(data, dtype=vd, count=nv, offset=end)
    off = end + nv * vd.itemsize
    fd = np.dtype([("n", "u1"), ("idx", "<i4", (3,))])
    faces = np.frombuffer(data, dtype=fd, count=nf, offset=off)
    assert off + nf * fd.itemsize == len(data) and (faces["n"] == 3).all()
    return verts["xyz"], faces["idx"], (verts["rgb"] if color else None)


def test_ply_round_trip(backend, tmp_path):
    from neuralsim_amd import mesh
    sdf = lambda x: torch.linalg.norm(x, dim=-1) - 0.5                       # noqa: E731
    col = lambda x, v: torch.cat([x * 2.0 + 0.5, (v[:, :1] + 1) * 0.5], dim=-1)[:, :3] * 1.5 - 0.2   # noqa: E731
    kw = dict(bmin=[-1, -1, -1], bmax=[1, 1, 1], N=20, show_progress=False, device=backend)
    plain = mesh.extract_mesh(sdf, filepath=str(tmp_path / "a.ply"), **kw)
    v, f, c = _read_ply(tmp_path / "a.ply")
    assert c is None and np.array_equal(v, plain["verts"]) and np.array_equal(f, plain["faces"]) and len(f) > 0
    T = np.array([[0.0, -1.0, 0.0, 1.0], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, 1.0, 0.5], [0.0, 0.0, 0.0, 1.0]])
    s = np.array([2.0, 3.0, 0.5])
    out = mesh.extract_mesh(sdf, col, include_color=True, scale=s, transform=T, filepath=str(tmp_path / "b.ply"), **kw)
    v2, f2, c2 = _read_ply(tmp_path / "b.ply")
    want = (plain["verts"].astype(np.float64) * s) @ T[:3, :3].T + T[:3, 3]
    assert np.abs(v2 - want).max() < 1e-5 and np.array_equal(f2, plain["faces"])
    cref = np.clip(col(torch.from_numpy(plain["verts"]), -torch.from_numpy(plain["normals"])).numpy(), 0, 1)
    assert c2.dtype == np.uint8 and np.abs(c2.astype(np.float64) - np.round(cref * 255)).max() <= 1
    assert c2.min() == 0 and c2.max() == 255                     # the clamp is exercised
    out3 = mesh.extract_mesh(sdf, scale=0.5, filepath=str(tmp_path / "c.ply"), **kw)
    assert np.abs(_read_ply(tmp_path / "c.ply")[0] - plain["verts"] * 0.5).max() < 1e-6
    assert out3["colors"] is None


# ------------------------------------------------------------------------------------------------ 7. reference tool
needs_reference = ref_glue.needs_reference(ref_glue.readable(CFG), reason="executes the reference's own sources, which only the authoring machine has (emulator backend)")


@needs_reference
def test_reference_extract_mesh_tool_runs_unchanged(backend, tmp_path):
    """``code_single/tools/extract_mesh.py``, source unchanged, on an experiment the reference's trainer wrote on this package:
    plain, and with ``--include_color --to_world``; the .ply files exist, parse, are closed and (second run) coloured."""
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    from test_reference_train import _run
    exp = tmp_path / "exp"
    r = _run(exp, ["--num_iters=4", "--training.i_val=-1", "--training.i_log=4"])
    assert r.returncode == 0 and "Everything done." in r.stdout, (r.stdout + r.stderr)[-3000:]
    env = dict(os.environ, PYTHONWARNINGS="ignore")
    for extra, dirname in (([], "m_plain"), (["--include_color", "--to_world"], "m_color")):
        cmd = [sys.executable, str(ROOT / "tools" / "run_reference_train.py"), "--emulate", "--script",
               "code_single/tools/extract_mesh.py", "--resume_dir", str(exp), "--N", "24", "--dirname", dirname] + extra
        rr = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=str(ROOT))
        assert rr.returncode == 0, (rr.stdout + rr.stderr)[-3000:]
        plys = list((exp / dirname).glob("*.ply"))
        assert len(plys) == 1, list((exp / dirname).iterdir())
        v, f, c = _read_ply(plys[0])
        assert len(f) > 0 and np.isfinite(v).all()
        _assert_closed(f)
        assert (c is not None) == bool(extra)
        if c is not None:
            assert c.shape == (len(v), 3) and c.std() > 0
