"""Visible grids (csrc/misc.hip ``nsim_vgrid_*``, neuralsim_amd/visible_grid.py) against the plain-torch restatement
tests/visible_grid_ref.py of ``app/visible_grid.py`` / ``code_multi/tools/extract_visible_grid.py:205-235``: marking from packed
volume buffers and from points, bit-identical voxel coordinates, the bit-packed morphology, the compaction, the reference's own
class (emulator) and its frozen results (both backends), the file, the driver over rendered views and the accel on a model.
Every comparison is exact: voxel sets are integers."""
import math
from pathlib import Path

import pytest
import torch

import ref_glue
import visible_grid_ref as vref
from util import look_at_cameras, make_params, model_from_params

FIXTURE = Path(__file__).resolve().parent / "golden" / "visible_grid_fixture.pt"
OPS = ("dilation", "close", "close2")
THRE = 0.1


def _space(aabb, backend):
    from neuralsim_amd.spatial import AABBSpace
    return AABBSpace(aabb=torch.as_tensor(aabb, dtype=torch.float32), device=backend)


def _grid(aabb, depth, backend):
    from neuralsim_amd.visible_grid import VisibleGrid
    return VisibleGrid(_space(aabb, backend), depth)


UNIT = [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]
# a street-shaped box, 2 : 1 : 0.3, away from the origin
LO = torch.tensor([0.3, -1.7, 2.2])
BOX = torch.stack([LO, LO + torch.tensor([2.0, 1.0, 0.3])])


# ------------------------------------------------------------------------------------------------ 1. marking
def _buffers(G, shift=0.0):
    """rays [R,3], and a packed buffer over a subset of them, built on the host:
    row 0: 150 samples (a ray spans waves) from outside the box through it and out again;  row 1: an empty pack;  row 2: a pack of
    1;  rows 3-5: three short packs inside one wave -- rays 5 and 6 sample the SAME voxel (a run may merge across the ray
    boundary), ray 7 another one (it must not);  row 6: 40 samples inside one voxel (step << voxel);  rows 7-9: points exactly
    on the lower faces, on the upper faces (clamped) and on a mixed corner.  Rays 1 and 4 are missed rays in between."""
    lo, hi = BOX[0], BOX[1]
    mid = (lo + hi) / 2
    vox = 2.0 / G
    z3 = torch.zeros(3)
    ex = torch.tensor([1.0, 0.0, 0.0])
    inner = lo + torch.tensor([0.52, 0.31, 0.11]) + shift
    rays = [
        (torch.stack([lo[0] - 0.5, mid[1] + shift, mid[2]]), ex),                  # 0
        (mid, ex),                                                                   # 1 (missed)
        (inner, torch.tensor([0.0, 1.0, 0.0])),                                      # 2 (empty pack)
        (inner, torch.tensor([0.3, 0.2, 0.1])),                                      # 3 (pack of 1)
        (mid, -ex),                                                                  # 4 (missed)
        (lo + (torch.tensor([7.0, 5.0, 1.0]) + 0.25) * vox, ex),                     # 5
        (lo + (torch.tensor([7.0, 5.0, 1.0]) + 0.30) * vox, ex),                     # 6: the same voxel as ray 5
        (lo + (torch.tensor([9.0, 5.0, 1.0]) + 0.30) * vox, ex),                     # 7: another voxel
        (lo + (torch.tensor([3.0, 2.0, 1.0]) + 0.1) * vox, torch.tensor([0.6, 0.5, 0.4])),   # 8: many samples in one voxel
        (lo.clone(), z3), (hi.clone(), z3), (torch.stack([hi[0], lo[1], hi[2]]), z3),         # 9, 10, 11
    ]
    rays_o = torch.stack([r[0] for r in rays]).float()
    rays_d = torch.stack([r[1] for r in rays]).float()
    rays_inds_hit = torch.tensor([0, 2, 3, 5, 6, 7, 8, 9, 10, 11])
    ts = [torch.linspace(0.0, 3.0, 150), torch.zeros(0), torch.tensor([0.4]), torch.arange(4) * vox * 0.1,
          torch.arange(3) * vox * 0.1, torch.arange(5) * vox * 0.1, torch.arange(40) * vox * 0.01, torch.tensor([0.0, 1.0]),
          torch.tensor([0.0, 2.0]), torch.tensor([0.5, 0.7])]
    lens = torch.tensor([len(t) for t in ts])
    pack_infos = torch.stack([torch.cumsum(lens, 0) - lens, lens], dim=-1)
    t = torch.cat(ts).float()
    w = torch.full_like(t, 0.5)
    # weights: exactly the threshold and NaN are not kept, the next float above the threshold is
    thre32 = torch.tensor(THRE, dtype=torch.float32)
    w[20:150:7] = thre32
    w[23:150:11] = float("nan")
    w[25:150:13] = torch.nextafter(thre32, torch.tensor(math.inf))
    w[3::17] = 0.05
    w[151], w[156], w[160] = thre32, float("nan"), 0.0
    return rays_o, rays_d, rays_inds_hit, pack_infos, t, w


def _ref_marking(bufs, depth, dev):
    idx = [vref.voxels_of_points(vref.points_of_samples(*[b.to(dev) for b in buf], thre=THRE), BOX.to(dev), depth) for buf in bufs]
    return vref.reduce(torch.cat(idx))


@pytest.mark.parametrize("G", [32, 64])
def test_marking_equals_restatement(backend, G):
    depth = int(math.log2(G))
    buf = _buffers(G)
    o, d, ri, pi, t, w = [b.to(backend) for b in buf]
    want_v, want_h = _ref_marking([buf], depth, backend)
    kept = (w > THRE)
    assert 0 < int(kept.sum()) < w.numel() and len(want_v) > 20 and int(want_h.max()) >= 30
    # some counted points lie on the upper faces: without the clamp their coordinate would be G
    pts = vref.points_of_samples(o, d, ri, pi, t, w, THRE)
    assert bool((pts == BOX[1].to(backend)).all(-1).any()) and bool((pts == BOX[0].to(backend)).all(-1).any())
    assert bool((pts[:, 0] < BOX[0, 0]).any()) and bool((pts[:, 0] > BOX[1, 0]).any())       # outside at both ends of ray 0
    g = _grid(BOX, depth, backend)
    assert g.add_samples(o, d, dict(type="packed", rays_inds_hit=ri, pack_infos_hit=pi, t=t, vw_normalized=w), thre=THRE) is None
    g.reduce_voxels()
    assert g.voxels_in_block[0].dtype == torch.int64 and g.voxel_hits_in_block[0].dtype == torch.int64
    assert torch.equal(g.voxels_in_block[0], want_v) and torch.equal(g.voxel_hits_in_block[0], want_h)
    # the fields instead of the dict; rays_inds_hit = None is the identity over the rows
    g2 = _grid(BOX, depth, backend)
    g2.add_samples(o[ri].contiguous(), d[ri].contiguous(), vw_normalized=w, t=t, pack_infos_hit=pi, thre=THRE)
    g2.reduce_voxels()
    assert torch.equal(g2.voxels_in_block[0], want_v) and torch.equal(g2.voxel_hits_in_block[0], want_h)
    # the same points as a point array
    g3 = _grid(BOX, depth, backend)
    frame = g3.reduce_points_and_add(pts, return_frame=True)
    assert g3.reduce_points_and_add(pts[:0]) is None
    g3.reduce_voxels()
    assert torch.equal(g3.voxels_in_block[0], want_v) and torch.equal(g3.voxel_hits_in_block[0], want_h)
    assert torch.equal(frame[0][0], want_v) and torch.equal(frame[1][0], want_h)


def test_two_calls_equal_one_call_over_the_concatenation(backend):
    depth, G = 5, 32
    a, b = _buffers(G), _buffers(G, shift=0.013)
    want_v, want_h = _ref_marking([a, b], depth, backend)
    g = _grid(BOX, depth, backend)
    for buf in (a, b):
        o, d, ri, pi, t, w = [x.to(backend) for x in buf]
        g.add_samples(o, d, vw_normalized=w, t=t, pack_infos_hit=pi, rays_inds_hit=ri, thre=THRE)
    g.reduce_voxels()
    assert torch.equal(g.voxels_in_block[0], want_v) and torch.equal(g.voxel_hits_in_block[0], want_h)
    R, S = a[0].shape[0], a[4].shape[0]
    o, d = torch.cat([a[0], b[0]]), torch.cat([a[1], b[1]])
    ri = torch.cat([a[2], b[2] + R])
    pi = torch.cat([a[3], b[3] + torch.tensor([S, 0])])
    t, w = torch.cat([a[4], b[4]]), torch.cat([a[5], b[5]])
    g1 = _grid(BOX, depth, backend)
    g1.add_samples(*[x.to(backend) for x in (o, d)], vw_normalized=w.to(backend), t=t.to(backend), pack_infos_hit=pi.to(backend),
                   rays_inds_hit=ri.to(backend), thre=THRE)
    g1.reduce_voxels()
    assert torch.equal(g1.voxels_in_block[0], want_v) and torch.equal(g1.voxel_hits_in_block[0], want_h)
    assert int(want_h.sum()) == int((a[5] > THRE).sum() + (b[5] > THRE).sum()) - _n_outside(a, b)


def _n_outside(*bufs):
    n = 0
    for buf in bufs:
        pts = vref.points_of_samples(*buf, thre=THRE)
        n += int((~((pts >= BOX[0]) & (pts <= BOX[1])).all(-1)).sum())
    return n


# ------------------------------------------------------------------------------------------------ 2. coordinates
def _ulp_steps(x: torch.Tensor, k: torch.Tensor) -> torch.Tensor:
    """x moved by k units in the last place (f32, positive and negative k; x away from zero)"""
    i = x.view(torch.int32) + torch.where(x >= 0, k, -k).to(torch.int32)
    return i.view(torch.float32)


@pytest.mark.parametrize("G", [32, 64])
def test_voxel_coordinates_are_bit_identical(backend, G):
    """Points whose ``(p - origin) / voxel_size`` lies within a few units in the last place of an integer, on both sides of it:
    the voxel must be the one the separate tensor operations give.  A fused multiply-add in ``o + d * t`` or an approximate
    division moves such a point across the voxel border."""
    depth = int(math.log2(G))
    lo = torch.tensor([0.3, -1.7, 2.2])
    box = torch.stack([lo, lo + torch.tensor([2.2, 1.1, 0.37])])           # voxel = 2.2 / G: no power of two
    gen = torch.Generator().manual_seed(G)
    n = 6000
    _, _, origin, voxel = vref.grid_of(box, depth)
    ext = (box[1] - box[0]).double()
    k = (torch.rand([n, 3], generator=gen).double() * (ext / voxel.double())).floor().clamp(min=1)
    target = (origin.double() + k * voxel.double()).float()                 # on a voxel border, to f32 rounding
    steps = torch.randint(-3, 4, [n, 3], generator=gen)
    pts = _ulp_steps(target, steps)
    q = (pts - origin) / voxel
    frac = q - q.round()
    assert int((frac < 0).sum()) > n // 2 and int((frac >= 0).sum()) > n // 2 and float(frac.abs().max()) < 1e-3
    # the same border points reached along rays: t solves o + d t = target on the x axis, then moves by units in the last place
    o = lo + torch.rand([n, 3], generator=gen) * (box[1] - box[0])
    d = torch.randn([n, 3], generator=gen)
    d = d / d.norm(dim=-1, keepdim=True)
    d[:, 0] = d[:, 0].abs().clamp(min=0.2) * torch.where(torch.rand([n], generator=gen) < 0.5, -1.0, 1.0)
    t = _ulp_steps(((target[:, 0].double() - o[:, 0].double()) / d[:, 0].double()).float(), steps[:, 0])
    dev = backend
    space = _space(box, dev)
    from neuralsim_amd.visible_grid import VisibleGrid
    g = VisibleGrid(space, depth)
    g.reduce_points_and_add(pts.to(dev))
    g.reduce_voxels()
    want_v, want_h = vref.reduce(vref.voxels_of_points(pts.to(dev), box.to(dev), depth))
    assert torch.equal(g.voxels_in_block[0], want_v) and torch.equal(g.voxel_hits_in_block[0], want_h)
    g = VisibleGrid(space, depth)
    pi = torch.stack([torch.arange(n), torch.ones(n, dtype=torch.long)], dim=-1)
    w = torch.ones(n)
    g.add_samples(o.to(dev), d.to(dev), vw_normalized=w.to(dev), t=t.to(dev), pack_infos_hit=pi.to(dev), thre=THRE)
    g.reduce_voxels()
    p_ray = vref.points_of_samples(o.to(dev), d.to(dev), None, pi.to(dev), t.to(dev), w.to(dev), THRE)
    want_v, want_h = vref.reduce(vref.voxels_of_points(p_ray, box.to(dev), depth))
    assert len(want_v) > 300
    assert torch.equal(g.voxels_in_block[0], want_v) and torch.equal(g.voxel_hits_in_block[0], want_h)


# ------------------------------------------------------------------------------------------------ 3. morphology
def _flat(G, *coords):
    c = torch.tensor(coords, dtype=torch.long).reshape(-1, 3)
    return (c[:, 0] * G + c[:, 1]) * G + c[:, 2]


def _sets(G):
    e = G - 1
    s = {"interior": _flat(G, (G // 2 + 1, G // 3, G // 2 - 3))}
    for i, c in enumerate([(x, y, z) for x in (0, e) for y in (0, e) for z in (0, e)]):
        s[f"corner{i}"] = _flat(G, c)
    # the ends of a row of words (z is the packed axis): nothing may leak into the next row (y + 1, z = 0) or come from the
    # previous one; at G = 64 the carry crosses the two words of a row at z = 31 | 32
    s["row_ends"] = _flat(G, (5, 7, e), (9, 3, 0), (12, e, e), (13, 0, 0), (4, 4, 31), (8, 8, 32 % G))
    yz = torch.cartesian_prod(torch.arange(G), torch.arange(G))
    s["face_x0"] = (0 * G + yz[:, 0]) * G + yz[:, 1]
    s["face_z_end"] = (yz[:, 0] * G + yz[:, 1]) * G + e
    gen = torch.Generator().manual_seed(G)
    s["random"] = torch.randperm(G ** 3, generator=gen)[:G ** 3 // 50].sort().values
    s["full"] = torch.arange(G ** 3)
    return s


@pytest.fixture(scope="module")
def morph_reference():
    """(G, set, op) -> voxels of the restatement, computed once on the host"""
    out = {}
    for G in (32, 64):
        for name, v in _sets(G).items():
            for op in OPS:
                out[G, name, op] = vref.postprocess(v, G, op)
    return out


@pytest.mark.parametrize("G", [32, 64])
def test_morphology_equals_restatement(backend, G, morph_reference):
    depth = int(math.log2(G))
    space = _space(UNIT, backend)
    from neuralsim_amd.visible_grid import VisibleGrid
    for name, v in _sets(G).items():
        for op in OPS:
            g = VisibleGrid(space, depth)
            g.voxels_in_block = {0: v.to(backend)}
            g.build_accel()
            assert g.postprocess(op) is g
            want = morph_reference[G, name, op].to(backend)
            assert torch.equal(g.voxels_in_block[0], want), (name, op, len(g.voxels_in_block[0]), len(want))
            # ... and the accel holds the same set, in its own (x fastest) order
            assert torch.equal(g.accel.occ_grid, vref.to_dense(want, G)), (name, op)
    full = morph_reference[G, "full", "close"]
    assert len(full) == G ** 3                       # erosion empties the border layer of a full grid, | orig restores it
    assert len(morph_reference[G, "corner0", "dilation"]) == 8 and len(morph_reference[G, "interior", "dilation"]) == 27


def test_morphology_steps_follow_the_reference_methods(backend):
    """``dilation_occ_grid`` / ``erosion_occ_grid`` / ``update_voxels_in_block_from_occgrid`` called one by one as
    ``postprocess("close")`` does (visible_grid.py:217-232)"""
    G = 32
    v = _sets(G)["random"].to(backend)
    g = _grid(UNIT, 5, backend)
    g.voxels_in_block = {0: v}
    g.build_accel()
    g.dilation_occ_grid()
    assert torch.equal(g.accel.occ_grid, vref.dilate(vref.to_dense(v, G)))
    g.erosion_occ_grid()
    g.update_voxels_in_block_from_occgrid()
    assert torch.equal(g.voxels_in_block[0], vref.postprocess(v, G, "close"))


# ------------------------------------------------------------------------------------------------ 4. compaction
def test_compaction_is_ascending_and_repeatable(backend):
    G = 64
    gen = torch.Generator().manual_seed(7)
    v = torch.randperm(G ** 3, generator=gen)[:G ** 3 // 50]                 # unsorted, 32 count blocks of 8192 voxels
    dense_words = torch.arange(40 * 32, 52 * 32 + 9)                          # ... whole words, up to 32 set bits each
    v = torch.cat([v, v[:100], dense_words])                                 # ... and repeats
    want = vref.to_dense(v, G).reshape(-1).nonzero()[:, 0]
    runs = []
    for _ in range(2):
        g = _grid(UNIT, 6, backend)
        g.voxels_in_block = {0: v.to(backend)}
        g.build_accel().update_voxels_in_block_from_occgrid()
        runs.append(g.voxels_in_block[0])
    assert torch.equal(runs[0], want.to(backend)) and torch.equal(runs[0], runs[1])
    assert bool((runs[0][1:] > runs[0][:-1]).all())
    e = _grid(UNIT, 6, backend).reduce_voxels()
    assert e.voxels_in_block[0].dtype == torch.int64 and e.voxels_in_block[0].shape == (0,)
    assert e.voxel_hits_in_block[0].dtype == torch.int64 and e.voxel_hits_in_block[0].shape == (0,)
    e.build_accel().postprocess("close2")
    assert e.voxels_in_block[0].shape == (0,) and not bool(e.accel.occ_grid.any())


# ------------------------------------------------------------------------------------------------ 5. the reference's class
needs_reference = ref_glue.needs_reference(ref_glue.readable(vref.REF_FILE),
                                           reason="executes the reference's own sources, which only the authoring machine has (emulator backend)")


def _product_run(pts, aabb, depth, op, backend):
    g = _grid(aabb, depth, backend)
    g.reduce_points_and_add(pts.to(backend))
    g.reduce_voxels()
    v, h = g.voxels_in_block[0].clone(), g.voxel_hits_in_block[0].clone()
    g.build_accel().postprocess(op)
    return v, h, g.voxels_in_block[0], g


@needs_reference
@pytest.mark.parametrize("op", OPS)
def test_reference_class_equals_restatement_and_product(backend, op, tmp_path):
    """``app/visible_grid.py``, source unchanged (its forest branch on one block over [0, 1]^3 -- the AABB branch does not run),
    at depth 5: ``reduce_points_and_add -> reduce_voxels -> build_accel -> postprocess(op)``"""
    f = torch.load(str(FIXTURE))
    pts, depth = f["pts"], f["octree_depth"]
    rv, rh, rpost = vref.run_reference(pts, depth, op)
    wv, wh = vref.reduce(vref.voxels_of_points(pts, f["aabb"], depth))
    assert torch.equal(rv, wv) and torch.equal(rh, wh) and torch.equal(rpost, vref.postprocess(wv, 2 ** depth, op))
    assert torch.equal(rv, f["voxels"]) and torch.equal(rpost, f["post"][op])            # the frozen copy is current
    pv, ph, ppost, g = _product_run(pts, f["aabb"], depth, op, backend)
    assert torch.equal(pv, rv) and torch.equal(ph, rh) and torch.equal(ppost, rpost)
    # a file written here loads in the reference's class
    g.save(str(tmp_path / "vg.pt"))
    ref_cls = vref.load_reference_class()
    back = ref_cls.load(str(tmp_path / "vg.pt"), vref.ForestBlockSpace())
    assert back.octree_depth == depth and torch.equal(back.voxels_in_block[0], rpost)


@pytest.mark.parametrize("op", OPS)
def test_frozen_reference_results(backend, op):
    """the recorded results of the reference's class (tests/golden/make_visible_grid_fixture.py), replayed on both backends"""
    f = torch.load(str(FIXTURE))
    pv, ph, ppost, _ = _product_run(f["pts"], f["aabb"], f["octree_depth"], op, backend)
    assert torch.equal(pv.cpu(), f["voxels"]) and torch.equal(ph.cpu(), f["hits"]) and torch.equal(ppost.cpu(), f["post"][op])
    assert len(f["voxels"]) > 200 and int(f["hits"].max()) > 1


# ------------------------------------------------------------------------------------------------ 6. file
def test_file_round_trip_and_a_file_of_the_reference(backend, tmp_path):
    from neuralsim_amd.visible_grid import VisibleGrid
    f = torch.load(str(FIXTURE))
    _, _, _, g = _product_run(f["pts"], f["aabb"], f["octree_depth"], "close", backend)
    path = str(tmp_path / "grid.pt")
    g.save(path)
    state = torch.load(path, map_location="cpu")
    assert set(state) == {"octree_depth", "voxels_in_block"} and state["octree_depth"] == 5 and type(state["octree_depth"]) is int
    assert list(state["voxels_in_block"]) == [0] and state["voxels_in_block"][0].dtype == torch.int64
    back = VisibleGrid.load(path, _space(f["aabb"], backend))
    assert back.octree_depth == 5 and torch.equal(back.voxels_in_block[0], g.voxels_in_block[0])
    # what the reference's ``save`` wrote
    ref_path = str(tmp_path / "ref.pt")
    torch.save(f["saved_state"], ref_path)
    theirs = VisibleGrid.load(ref_path, _space(f["aabb"], backend))
    assert torch.equal(theirs.voxels_in_block[0].cpu(), f["post"]["close"])
    theirs.build_accel().postprocess("dilation")           # the reference flow: load -> build_accel -> postprocess
    assert torch.equal(theirs.voxels_in_block[0].cpu(), vref.postprocess(f["post"]["close"], 32, "dilation"))
    assert theirs.reduce_voxels() is theirs and len(theirs.voxels_in_block[0]) > 0         # nothing was added: kept


# ------------------------------------------------------------------------------------------------ 7. driver and accel
QP = dict(nablas_has_grad=False, num_coarse=16, num_fine=[4, 4, 8], upsample_inv_s=64.0, upsample_inv_s_factors=[1, 4, 16],
          upsample_use_estimate_alpha=True, march_cfg=dict(step_size=0.08, max_steps=128))
MARCH_ONLY = dict(QP, num_coarse=0, num_fine=[], march_cfg=dict(step_size=0.02, max_steps=512))
_VIEWS = dict(V=2, radius=3.0, H=32, W=32, f=36.0, seed=1)


def _sphere_model(backend, qp=QP):
    m = model_from_params(make_params(sphere=True), backend)
    m.ray_query_cfg = dict(query_mode="march_occ_multi_upsample", query_param=qp)
    return m


def test_grid_from_views_equals_restatement(backend):
    from neuralsim_amd import visible_grid as vg
    from neuralsim_amd.eval import all_pixel_xy
    from neuralsim_amd.graphics.cameras import selected_rays
    m = _sphere_model(backend)
    intr, c2w, WH = [x.to(backend) for x in look_at_cameras(**_VIEWS)]
    chunk = 400                                                        # 1024 rays per view: the last chunk is short
    grid = vg.visible_grid_from_views(m, intr, c2w, WH, [0, 1], rayschunk=chunk, octree_depth=5)
    idx = []
    n_kept = n_missed = 0
    with torch.no_grad():
        for frame in (0, 1):
            xy = all_pixel_xy(32, 32, backend)
            o, d = selected_rays(xy, torch.full([1024], frame, dtype=torch.long, device=backend), intr, c2w, WH)
            for i in range(0, 1024, chunk):
                oc, dc = o[i:i + chunk].contiguous(), d[i:i + chunk].contiguous()
                vb = vg.view_buffers(m, oc, dc, forward_inv_s=64000.)
                assert vb is not None
                n_missed += oc.shape[0] - vb["rays_inds_hit"].shape[0]
                pts = vref.points_of_samples(oc, dc, vb["rays_inds_hit"], vb["pack_infos_hit"], vb["t"], vb["vw_normalized"], 0.1)
                n_kept += pts.shape[0]
                idx.append(vref.voxels_of_points(pts, m.space.aabb, 5))
    want_v, want_h = vref.reduce(torch.cat(idx))
    print(f"driver: {n_kept} kept samples, {len(want_v)} voxels, {n_missed} rays outside the buffers")
    assert len(want_v) > 60 and int(want_h.sum()) == n_kept and n_missed > 0
    assert torch.equal(grid.voxels_in_block[0], want_v) and torch.equal(grid.voxel_hits_in_block[0], want_h)
    # the observed surface is the sphere of radius 0.5: every voxel centre within a voxel diagonal (+ one marching step) of it
    c = vg.voxel_indices_to_voxel_coords(want_v, grid.grid_size).float()
    ctr = grid.grid_center + (c + 0.5) * grid.voxel_size
    assert float((ctr.norm(dim=-1) - 0.5).abs().max()) <= math.sqrt(3.0) / 16 + 0.08
    # the tool's inference of the voxel size: twice the ray gap at the far plane
    size = vg.infer_voxel_size(intr, far=4.0)
    assert size == pytest.approx(2 * 4.0 * math.sqrt(2) / 36.0, rel=1e-6)
    assert vg.VisibleGrid(m.space, prefer_voxel_size=2.0 / 40).octree_depth == 5           # floor(log2(40))


def test_model_marches_the_visible_grid_and_prunes_by_it(backend):
    from neuralsim_amd import occgrid
    from neuralsim_amd import visible_grid as vg
    from neuralsim_amd.eval import all_pixel_xy
    from neuralsim_amd.graphics.cameras import selected_rays
    m = _sphere_model(backend)
    intr, c2w, WH = [x.to(backend) for x in look_at_cameras(**_VIEWS)]
    grid = vg.visible_grid_from_views(m, intr, c2w, WH, [0, 1], rayschunk=1024, octree_depth=5)
    full = occgrid.extract_occupancy_from_model(m, occ_res=2.0 / 24 - 1e-4, subsample_factor=1)
    grid.build_accel().postprocess("close2")
    m.accel = grid.accel
    dense = vref.to_dense(grid.voxels_in_block[0], 32)
    assert torch.equal(m.accel.occ_grid, dense) and torch.equal(m.space.aabb, grid.space.aabb)
    # pure marching: every sample is a marching step the kernels tested against the grid's bits
    m.ray_query_cfg = dict(query_mode="march_occ_multi_upsample", query_param=MARCH_ONLY)
    n = 0
    with torch.no_grad():
        xy = all_pixel_xy(32, 32, backend)
        o, d = selected_rays(xy, torch.zeros([1024], dtype=torch.long, device=backend), intr, c2w, WH)
        tested = m.ray_test(o, d)
        ret = m.ray_query(ray_tested=tested, config=dict(m.ray_query_cfg, perturb=False, with_rgb=False), return_details=True)
        vb = ret["volume_buffer"]
        ridx = ret["details"]["ridx"]
        x = tested["rays_o"][ridx] + tested["rays_d"][ridx] * vb["t"][:, None]
        n = x.shape[0]
        assert n > 500 and int(vb["pack_infos_hit"][:, 1].sum()) == n
        cells = vref.voxels_of_points(x, m.space.aabb, 5)
        assert cells.shape[0] == n and bool(dense.reshape(-1)[cells].all())
        assert bool(m.accel.occ_val[occgrid.accel_cells_of(m.accel, x)].eq(1.0).all())
        # ... and rays are still tested against the model's box
        assert tested["num_rays"] == m.space.ray_test(o, d)["num_rays"]
    pruned = occgrid.extract_occupancy_from_model(m, occ_res=2.0 / 24 - 1e-4, subsample_factor=1, prune="accel")
    f = set(map(tuple, full["occ_corners"].cpu().tolist()))
    p = set(map(tuple, pruned["occ_corners"].cpu().tolist()))
    assert p <= f and 0 < len(p) and pruned["stats"]["n_queried"] < full["stats"]["n_queried"]


def test_accel_of_a_non_cubic_space_keeps_the_box(backend):
    """the accel spans the cube, the model's box stays the space's: ``aabb`` and the ray-test meta are the box"""
    g = _grid(BOX, 5, backend)
    g.voxels_in_block = {0: _flat(32, (3, 2, 1)).to(backend)}
    g.build_accel()
    a = g.accel
    assert torch.equal(a.aabb.cpu(), BOX) and a.resolution == [32, 32, 32]
    lo, hi = g.get_grid_aabb_in_world()
    assert torch.equal(a.grid_aabb, torch.stack([lo, hi])) and torch.equal(lo.cpu(), BOX[0])
    assert float(hi[0] - lo[0]) == pytest.approx(2.0) and float(hi[2] - lo[2]) == pytest.approx(2.0)
    assert [a.meta.aabb_max[i] for i in range(3)] == [float(v) for v in hi] and a.meta.res[0] == 32
    assert [a.box_meta.aabb_max[i] for i in range(3)] == [float(v) for v in BOX[1]]
    assert 0.0 < a.occ_thre < 1.0
    a.cur_batch__step(10 ** 6, lambda x: x[:, 0])                       # no training hook refreshes it
    a.init(lambda x: x[:, 0])
    assert int(a.occ_grid.sum()) == 1 and bool(a.occ_grid[3, 2, 1])
    mins, maxs = g.get_voxel_aabb_in_world(g.voxels_in_block[0])
    want = BOX[0].to(backend) + torch.tensor([3.0, 2.0, 1.0], device=backend) * g.voxel_size_in_world
    assert torch.allclose(mins[0], want) and torch.allclose(maxs[0] - mins[0], g.voxel_size_in_world)
    idx = g.voxels_in_block[0]
    from neuralsim_amd.visible_grid import voxel_coords_to_voxel_indices, voxel_indices_to_voxel_coords
    assert torch.equal(voxel_coords_to_voxel_indices(voxel_indices_to_voxel_coords(idx, g.grid_size), g.grid_size), idx)


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals(backend):
    from neuralsim_amd.visible_grid import VisibleGrid
    space = _space(UNIT, backend)
    for depth in (4, 11):
        with pytest.raises(ValueError, match="octree_depth"):
            VisibleGrid(space, depth)
    with pytest.raises(ValueError, match="octree_depth"):
        VisibleGrid(space, prefer_voxel_size=0.25)                   # floor(log2(4)) = 2
    with pytest.raises(ValueError, match="prefer_voxel_size"):
        VisibleGrid(space)
    ForestBlockSpace = type("ForestBlockSpace", (), {})
    with pytest.raises(NotImplementedError, match="ForestBlockSpace"):
        VisibleGrid(ForestBlockSpace(), 5)
    g = VisibleGrid(space, 5)
    for call in (lambda: g.postprocess("close"), g.dilation_occ_grid, g.erosion_occ_grid, g.update_voxels_in_block_from_occgrid):
        with pytest.raises(RuntimeError, match="build_accel"):
            call()
    g.build_accel()
    with pytest.raises(AssertionError, match="Only support dilation, close, close2 operation"):
        g.postprocess("open")
    with pytest.raises(NotImplementedError, match="packed"):
        g.add_samples(torch.zeros([1, 3], device=backend), torch.zeros([1, 3], device=backend), dict(type="batched"))
    with pytest.raises(RuntimeError, match="code 57"):
        from neuralsim_amd import _lib
        _lib.call("nsim_vgrid_count", _lib.ptr(torch.zeros([8], dtype=torch.int32, device=backend)), 16,
                  _lib.ptr(torch.zeros([1], dtype=torch.int32, device=backend)))


def test_refuses_host_tensors():
    from neuralsim_amd.visible_grid import VisibleGrid
    from neuralsim_amd.spatial import AABBSpace
    with pytest.raises(RuntimeError, match="no CPU path"):
        VisibleGrid(AABBSpace(aabb=torch.tensor(UNIT)), 5)


@pytest.mark.gpu
def test_methods_refuse_host_tensors():
    g = _grid(UNIT, 5, torch.device("cuda"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        g.reduce_points_and_add(torch.rand([4, 3]))
    z = torch.zeros([1, 3])
    with pytest.raises(RuntimeError, match="no CPU path"):
        g.add_samples(z, z, vw_normalized=torch.ones([1]), t=torch.ones([1]), pack_infos_hit=torch.tensor([[0, 1]]))
    g.voxels_in_block = {0: torch.tensor([5])}
    with pytest.raises(RuntimeError, match="no CPU path"):
        g.build_accel()
