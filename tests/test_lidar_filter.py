"""The LiDAR ground-truth filter and the camera projection (neuralsim_amd/lidar_filter.py on ``nsim_lidar_filter_count / _emit`` and
``nsim_cam_project``, csrc/misc.hip) against tests/lidar_filter_ref.py: every decision against the rule in float64 with the
reference's own f32 torch composition as the yardstick, the exact compaction, each filter alone and all together, exactly
constructed edge points, the projection tuple, bank = frames, the replay of the reference's frozen outputs
(tests/golden/lidar_filter_fixture.pt), the adapter for the reference's loader, the trainer hook, and the refusals.

Margins.  A decision quantity q (u, v, d, the AABB and box coordinates) has the margin 2 x max |f32 composition - float64| on the
same inputs (``lidar_filter_ref.margins``; the factor and its reasoning are test_lidar_sim.py's).  A point is *undecidable* when a
float64 quantity lies within its margin of a threshold (or its ignore-mask pixel could become one of another value); everywhere
else the kernel must decide as float64 does.  Measured over the cases of this file: DESIGN.md, "LiDAR ground-truth filter"."""
import contextlib
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import lidar_filter_ref as fref
import ref_glue
from neuralsim_amd import _lib as _product_lib

_REQUIRE_DEVICE = _product_lib.require_device          # the product's own check (the emulator backend patches it away)
GOLDEN = Path(__file__).resolve().parent / "golden" / "lidar_filter_fixture.pt"
MAX_UNDECIDABLE = 0.005
MIN_IN_VIEW = 0.02

MODELS5 = ["pinhole", "opencv", "fisheye", "opencv", "pinhole"]
HW5 = [(64, 96), (48, 80), (64, 96), (48, 80), (64, 96)]
DIST = {"pinhole": [0.0, 0.0, 0.0, 0.0, 0.0], "opencv": [-0.05, 0.01, 0.001, -0.0015, 0.0005],
        "fisheye": [0.02, -0.003, 0.0008, -0.0001, 0.0]}


def _dev(t: torch.Tensor, backend) -> torch.Tensor:
    """a copy in a NaN-poisoned ``torch.empty`` buffer on the backend's device"""
    out = torch.empty(list(t.shape), dtype=t.dtype, device=backend)
    out.copy_(t)
    return out


def _rodrigues(ax, a):
    ax = torch.as_tensor(ax, dtype=torch.float64)
    ax = ax / ax.norm()
    K = torch.tensor([[0.0, -ax[2], ax[1]], [ax[2], 0.0, -ax[0]], [-ax[1], ax[0], 0.0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)


def _rand_pose(g, spread):
    R = _rodrigues(torch.randn(3, generator=g, dtype=torch.float64), float(torch.rand(1, generator=g)) * 2 * math.pi)
    t = (torch.rand(3, generator=g, dtype=torch.float64) * 2 - 1) * spread
    return torch.cat([R, t[:, None]], dim=1)


def _frame_cuts(N, F):
    """frame boundaries inside a 256-point block and inside a 64-lane wave (never on a multiple of 64 unless N forces it)"""
    cuts = [0]
    for f in range(1, F):
        c = (N * f) // F
        c += 17 if (c + 17) % 64 and c + 17 < N else 0
        cuts.append(min(max(c, cuts[-1]), N))
    return cuts + [N]


def make_scene(N, C, L, F, nbox, seed, ignore=True, aabb=True, invalid=0.1):
    """points uniform in a +-60 m cube around a C-camera rig with distinct rotations and mixed models (OpenCV with all five
    coefficients and a skew), L lidars per frame, F frames, ``nbox`` rotated anisotropic boxes per frame (frame 1 of a sequence
    carries none)"""
    g = torch.Generator().manual_seed(seed)
    models = MODELS5[:C]
    hw = torch.tensor(HW5[:C], dtype=torch.long)
    c2w, intr, dist = [], [], []
    for f in range(F):
        shift = torch.tensor([3.0 * f, 0.5 * f, 0.1 * f], dtype=torch.float64)
        for c in range(C):
            m = _rand_pose(g, 1.5)
            m[:, 3] += shift
            c2w.append(m)
            H, W = HW5[c]
            fx = 0.45 * W
            intr.append(torch.tensor([[fx, 0.7 if models[c] == "opencv" else 0.0, W / 2 + 0.3], [0.0, 1.05 * fx, H / 2 - 0.2],
                                      [0.0, 0.0, 1.0]], dtype=torch.float64))
            dist.append(torch.tensor(DIST[models[c]], dtype=torch.float64))
    cams = dict(c2w=torch.stack(c2w).view(F, C, 3, 4).float(), intr=torch.stack(intr).view(F, C, 3, 3).float(), hw=hw, models=models,
                dist=torch.stack(dist).view(F, C, 5).float())
    l2w = torch.stack([_rand_pose(g, 2.0) for _ in range(F * L)]).view(F, L, 3, 4)
    for f in range(F):
        l2w[f, :, 0, 3] += 3.0 * f
    l2w = l2w.float()
    cuts = _frame_cuts(N, F)
    fi = torch.cat([torch.full((cuts[f + 1] - cuts[f],), f, dtype=torch.long) for f in range(F)]) if N else torch.zeros(0, dtype=torch.long)
    li = torch.randint(0, L, (N,), generator=g)
    # world targets uniform in the cube -> the lidar's frame (float64) -> origin, unit direction, range, rounded to f32
    P = (torch.rand(N, 3, generator=g, dtype=torch.float64) * 2 - 1) * 60.0
    m64 = l2w.double()[fi, li]
    pl = ((P - m64[:, :, 3]).unsqueeze(-2) * m64[:, :, :3].transpose(-1, -2)).sum(-1)
    o = (torch.rand(N, 3, generator=g, dtype=torch.float64) - 0.5)
    rng = (pl - o).norm(dim=-1)
    d = (pl - o) / rng.clamp_min(1e-9).unsqueeze(-1)
    rng = rng.float()
    bad = torch.tensor([0.0, -0.0, -1.0, float("nan")])
    pick = torch.rand(N, generator=g) < invalid
    rng[pick] = bad[torch.randint(0, 4, (N,), generator=g)][pick]
    sc = dict(rays_o=o.float(), rays_d=d.float(), ranges=rng, l2w=l2w, cams=cams, filter_valid=True, near_clip=1e-4)
    if L > 1:
        sc["li"] = li
    else:
        sc["l2w"] = l2w
    if F > 1:
        sc["fi"] = fi
    if ignore:                            # a few large rectangles: mask edges are rare
        Hm, Wm = int(hw[:, 0].max()), int(hw[:, 1].max())
        ign = torch.zeros(F, C, Hm, Wm, dtype=torch.bool)
        for f in range(F):
            for c in range(C):
                H, W = HW5[c]
                ign[f, c, 10:30, 20 + 3 * c:50 + f] = True
                ign[f, c, 40:H, :15] = True
        sc["ignore"] = ign
    if aabb:
        sc["aabb"] = torch.tensor([[-40.0, -45.0, -30.0], [45.0, 40.0, 35.0]])
    if nbox is not None:
        rows, off = [], [0]
        for f in range(F):
            n = 0 if (F > 1 and f == 1) else nbox
            for _ in range(n):
                m = _rand_pose(g, 40.0)
                s = 4.0 + 21.0 * torch.rand(3, generator=g, dtype=torch.float64)
                rows.append(torch.cat([m.reshape(-1), s]))
            off.append(off[-1] + n)
        sc["boxes"] = torch.stack(rows).float() if rows else torch.zeros(0, 15)
        sc["box_offsets"] = torch.tensor(off, dtype=torch.int32)
    return sc


def _subscene(sc, valid=True, cams=True, aabb=True, objs=True, ignore=True):
    out = {k: v for k, v in sc.items() if k in ("rays_o", "rays_d", "ranges", "li", "fi", "l2w", "near_clip")}
    out["filter_valid"] = valid
    if cams:
        out["cams"] = sc["cams"]
        if ignore and "ignore" in sc:
            out["ignore"] = sc["ignore"]
    if aabb and "aabb" in sc:
        out["aabb"] = sc["aabb"]
    if objs and "boxes" in sc:
        out["boxes"], out["box_offsets"] = sc["boxes"], sc["box_offsets"]
    return out


def _camera_set(sc, backend, frame=None):
    from neuralsim_amd import lidar_filter as lf
    c = sc["cams"]
    F = c["c2w"].shape[0]
    if frame is None and F > 1:
        return lf.CameraSet(_dev(c["c2w"], backend), _dev(c["intr"], backend), c["hw"].expand(F, *c["hw"].shape), c["models"],
                            _dev(c["dist"], backend))
    f = frame or 0
    if "raw" in c:
        intr, hw, ds = c["raw"]
        return lf.CameraSet(_dev(c["c2w"][f].contiguous(), backend), _dev(intr.contiguous(), backend), hw, c["models"],
                            _dev(c["dist"][f].contiguous(), backend), downscale=ds)
    return lf.CameraSet(_dev(c["c2w"][f].contiguous(), backend), _dev(c["intr"][f].contiguous(), backend), c["hw"], c["models"],
                        _dev(c["dist"][f].contiguous(), backend))


def _data(sc, backend, sel=slice(None), extra=None):
    d = {k: _dev(sc[k][sel].contiguous(), backend) for k in ("rays_o", "rays_d", "ranges")}
    if "li" in sc:
        d["li"] = _dev(sc["li"][sel].contiguous(), backend)
    for k, v in (extra or {}).items():
        d[k] = _dev(v[sel].contiguous(), backend)
    return d


def run_filter(sc, backend, extra=None, **kw):
    """the scene through ``filter_lidar`` (one frame) or ``filter_lidar_bank`` (a sequence, flat with frame_inds)"""
    from neuralsim_amd import lidar_filter as lf
    F = sc["l2w"].shape[0]
    args = dict(filter_valid=sc.get("filter_valid", True), near_clip=sc.get("near_clip", 1e-4), **kw)
    if sc.get("cams") is not None:
        args["cams"] = _camera_set(sc, backend)
        if sc.get("ignore") is not None:
            args["ignore_mask"] = _dev(sc["ignore"] if F > 1 else sc["ignore"][0], backend)
    if sc.get("aabb") is not None:
        args["aabb"] = _dev(sc["aabb"], backend)
    if sc.get("boxes") is not None:
        args["boxes"] = _dev(sc["boxes"], backend)
        args["box_offsets"] = _dev(sc["box_offsets"], backend)
    l2w = sc["l2w"] if "li" in sc else sc["l2w"][:, 0]
    if F > 1:
        return lf.filter_lidar_bank(_data(sc, backend, extra=extra), _dev(l2w.contiguous(), backend),
                                    frame_inds=_dev(sc["fi"], backend), **args)
    return lf.filter_lidar(_data(sc, backend, extra=extra), _dev(l2w[0].contiguous(), backend), **args)


def _keep_mask(out, N):
    k = torch.zeros(N, dtype=torch.bool)
    k[out["keep_inds"].cpu()] = True
    return k


_ANALYSIS = {}


def _scene(N, C, L, F, nbox, seed=None):
    """scenes and their float64 / f32 analysis are computed once and shared, unchanged, between the tests"""
    key = (N, C, L, F, nbox, seed)
    if key not in _ANALYSIS:
        sc = make_scene(N, C, L, F, nbox, seed if seed is not None else 1000 + N + 7 * C + 13 * L + 31 * F + (nbox or 0))
        _ANALYSIS[key] = (sc, fref.analyse(sc))
    return _ANALYSIS[key]


# ------------------------------------------------------------------------------------------------ 1. decisions against float64
CASES = [(0, 5, 1, 1, 1), (1, 1, 1, 1, 0), (63, 5, 5, 1, 1), (257, 1, 1, 3, 70), (1000, 5, 5, 3, 70), (1000, 1, 5, 1, 0),
         (20000, 5, 5, 3, 70), (20000, 5, 1, 1, 1)]


@pytest.mark.parametrize("N,C,L,F,nbox", CASES)
def test_decisions_equal_float64_on_decidable_points(backend, N, C, L, F, nbox):
    sc, an = _scene(N, C, L, F, nbox)
    out = run_filter(sc, backend, return_inds=True)
    keep = _keep_mask(out, N)
    und, k64, k32 = an["und"], an["dec64"]["keep"], an["dec32"]["keep"]
    share = float(und.float().mean()) if N else 0.0
    seen = an["dec64"]["view"].float().mean(1) if N else torch.ones(C)
    print(f"lidar filter N {N} C {C} L {L} F {F} boxes {nbox}: margins " + " ".join(f"{k} {v:.3e}" for k, v in an["margins"].items())
          + f" | undecidable {share:.2e} kept {int(k64.sum())} in view per camera " + " ".join(f"{float(s):.3f}" for s in seen)
          + f" | kernel != f64 on {int((keep != k64).sum())}, f32 != f64 on {int((k32 != k64).sum())}")
    assert int(out["ranges"].shape[0]) == int(keep.sum())
    assert bool((keep == k64)[~und].all()), (keep != k64).nonzero()[:8]
    assert bool((k32 == k64)[~und].all())
    assert share <= MAX_UNDECIDABLE
    if N >= 1000:                       # (a share of in-view points means nothing for a handful of points)
        assert float(seen.min()) >= MIN_IN_VIEW, seen
        assert 0.02 * N < int(k64.sum()) < 0.9 * N


# ------------------------------------------------------------------------------------------------ 2. compaction is exact
def _world_f32(sc):
    """the stated order, one rounded f32 operation at a time"""
    o, d, r = sc["rays_o"], sc["rays_d"], sc["ranges"]
    N = o.shape[0]
    li = sc.get("li", torch.zeros(N, dtype=torch.long))
    fi = sc.get("fi", torch.zeros(N, dtype=torch.long))
    q = o + d * r.unsqueeze(-1)
    m = sc["l2w"][fi, li]
    return torch.stack([((m[:, k, 0] * q[:, 0] + m[:, k, 1] * q[:, 1]) + m[:, k, 2] * q[:, 2]) + m[:, k, 3] for k in range(3)], dim=-1)


@pytest.mark.parametrize("N,C,L,F,nbox", [(1000, 5, 5, 1, 1), (1000, 5, 5, 3, 70), (257, 1, 1, 3, 70), (1, 1, 1, 1, 0), (0, 5, 1, 1, 1)])
def test_compaction_is_exact(backend, N, C, L, F, nbox):
    sc, _ = _scene(N, C, L, F, nbox)
    g = torch.Generator().manual_seed(5)
    extra = dict(intensity=torch.rand(N, generator=g), rgb=torch.rand(N, 3, generator=g), ring=torch.randint(0, 64, (N,), generator=g))
    full = run_filter(sc, backend, extra=extra, return_inds=True, return_pts=True)
    inds = full["keep_inds"].cpu()
    assert inds.dtype == torch.long and bool((inds[1:] > inds[:-1]).all())                      # point order
    for k in ("rays_o", "rays_d", "ranges", "li", "intensity", "rgb", "ring"):
        if k in full:
            src = sc[k] if k in sc else extra[k]
            assert fref.copies_equal(full[k].cpu(), src[inds]), k
    assert fref.copies_equal(full["pts_world"].cpu(), _world_f32(sc)[inds])
    if F > 1:
        assert fref.copies_equal(full["frame_inds"].cpu(), sc["fi"][inds])
    plain = run_filter(sc, backend, extra=extra)
    assert "keep_inds" not in plain and "pts_world" not in plain
    assert list(plain.keys())[:len(plain) - (2 if F > 1 else 0)] == list(_data(sc, torch.device("cpu"), extra=extra).keys())
    for k in plain:
        assert fref.copies_equal(plain[k].cpu(), full[k].cpu()), k
    only_pts = run_filter(sc, backend, return_pts=True)
    assert "keep_inds" not in only_pts and fref.copies_equal(only_pts["pts_world"].cpu(), full["pts_world"].cpu())


# ------------------------------------------------------------------------------------------------ 3. each filter alone, all together
FLAG_SETS = [dict(valid=True, cams=False, aabb=False, objs=False), dict(valid=False, cams=True, aabb=False, objs=False),
             dict(valid=False, cams=True, aabb=False, objs=False, ignore=False), dict(valid=False, cams=False, aabb=True, objs=False),
             dict(valid=False, cams=False, aabb=False, objs=True), dict(valid=False, cams=False, aabb=False, objs=False),
             dict(valid=True, cams=True, aabb=True, objs=True)]


@pytest.mark.parametrize("F", [1, 3])
def test_each_filter_alone_and_all_together(backend, F):
    """every selection of filters equals the reference's sequential application (mask, nonzero, gather, one after another) of the
    rule in float64; a frame with zero boxes keeps everything"""
    base, _ = _scene(1000, 5, 5, F, 70)
    for flags in FLAG_SETS:
        sc = _subscene(base, **flags)
        an = fref.analyse(sc)
        out = run_filter(sc, backend, return_inds=True)
        got = out["keep_inds"].cpu()
        want, _ = fref.sequential_filter(sc, an["q64"])
        ok = ~an["und"]
        assert torch.equal(got[ok[got]], want[ok[want]]), flags
        assert float(an["und"].float().mean()) <= MAX_UNDECIDABLE
        if not any(flags[k] for k in ("valid", "cams", "aabb", "objs")):
            assert got.numel() == 1000
        if flags["objs"] and not (flags["valid"] or flags["cams"] or flags["aabb"]):
            assert 0 < got.numel() < 1000
            if F == 3:                   # frame 1 carries no box: every one of its points stays
                f1 = (base["fi"] == 1).nonzero()[:, 0]
                assert torch.equal(got[base["fi"][got] == 1], f1)
    sc = _subscene(base, valid=False, cams=False, aabb=False, objs=True)
    sc["boxes"], sc["box_offsets"] = torch.zeros(0, 15), torch.zeros(F + 1, dtype=torch.int32)
    assert run_filter(sc, backend)["ranges"].shape[0] == 1000


# ------------------------------------------------------------------------------------------------ 4. adversarial points
def _points_scene(pts, ranges=None, **kw):
    """points given in the world: origin = the point, direction 0, identity pose -> the world point is the point, bit for bit"""
    n = pts.shape[0]
    sc = dict(rays_o=pts.float(), rays_d=torch.zeros(n, 3), ranges=torch.ones(n) if ranges is None else ranges,
              l2w=torch.eye(4)[:3].reshape(1, 1, 3, 4).clone(), filter_valid=False, near_clip=1e-4)
    sc.update(kw)
    return sc


def _pinhole_cam():
    """identity pose, fx = fy = 32, cx = 32, cy = 24, no skew, 64 x 48: u = 32 x / z + 32 is exact for the points below"""
    return dict(c2w=torch.eye(4)[:3].reshape(1, 1, 3, 4).clone(), intr=torch.tensor([[32.0, 0.0, 32.0], [0.0, 32.0, 24.0],
                                                                                     [0.0, 0.0, 1.0]]).reshape(1, 1, 3, 3),
                hw=torch.tensor([[48, 64]]), models=["pinhole"], dist=torch.zeros(1, 1, 5))


def test_adversarial_points(backend):
    inf, nan = float("inf"), float("nan")
    pts = torch.tensor([[0.0, 0.0, 5.0],          # 0 plainly in view
                        [0.0, 0.0, -5.0],         # 1 behind the camera (d < 0)
                        [0.0, 0.0, 0.0],          # 2 z == 0 exactly: the guard, d = 0 is not beyond the near plane
                        [-2.0, 0.0, 2.0],         # 3 u == 0.0 exactly: in view
                        [2.0, 0.0, 2.0],          # 4 u == W exactly: out
                        [0.0, -1.5, 2.0],         # 5 v == 0.0 exactly: in view
                        [0.0, 1.5, 2.0],          # 6 v == H exactly: out
                        [nan, 0.0, 5.0], [0.0, nan, 5.0], [0.0, 0.0, nan],                       # 7 8 9
                        [inf, 0.0, 5.0], [0.0, -inf, 5.0], [0.0, 0.0, inf], [0.0, 0.0, -inf],    # 10 11 12 13
                        [1e30, 1e30, 1e-3],       # 14 a pixel coordinate beyond every integer range
                        [0.5, 0.25, 2.0]])        # 15 in view, on an ignored pixel (u = 40, v = 28)
    ign = torch.zeros(1, 1, 48, 64, dtype=torch.bool)
    ign[0, 0, 28, 40] = True
    for with_ignore, want in ((False, [0, 3, 5, 15]), (True, [0, 3, 5])):
        sc = _points_scene(pts, cams=_pinhole_cam(), **(dict(ignore=ign) if with_ignore else {}))
        out = run_filter(sc, backend, return_inds=True)
        assert out["keep_inds"].cpu().tolist() == want, with_ignore
        assert fref.decide(sc, fref.quantities(sc, torch.float64))["keep"].nonzero()[:, 0].tolist() == want
    # ranges: only range > 0 is valid
    r = torch.tensor([0.0, -0.0, -1.0, nan, 1e-30, 7.5, inf])
    sc = _points_scene(torch.zeros(7, 3), ranges=r, filter_valid=True)
    assert run_filter(sc, backend, return_inds=True)["keep_inds"].cpu().tolist() == [4, 5, 6]
    # a box face is inclusive (the point is removed), one f32 step outside it is not
    up = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
    box = torch.tensor([[1.0, 0, 0, 0.0, 0, 1.0, 0, 0.0, 0, 0, 1.0, 20.0, 2.0, 4.0, 6.0]])
    pts = torch.tensor([[1.0, 0.0, 20.0], [up, 0.0, 20.0], [-1.0, 2.0, 23.0], [-up, 2.0, 23.0], [0.0, 0.0, 20.0], [0.0, 0.0, 0.0],
                        [nan, 0.0, 20.0]])
    sc = _points_scene(pts, boxes=box, box_offsets=torch.tensor([0, 1], dtype=torch.int32))
    assert run_filter(sc, backend, return_inds=True)["keep_inds"].cpu().tolist() == [1, 3, 5, 6]
    # an AABB face is inclusive (the point is kept)
    aabb = torch.tensor([[-1.0, -1.0, -1.0], [3.0, 3.0, 30.0]])
    up3 = float(np.nextafter(np.float32(3.0), np.float32(4.0)))
    pts = torch.tensor([[3.0, 0.0, 0.0], [up3, 0.0, 0.0], [-1.0, -1.0, -1.0], [0.0, -up, 0.0], [3.0, 3.0, 30.0], [0.0, nan, 0.0],
                        [0.0, 0.0, inf]])
    sc = _points_scene(pts, aabb=aabb)
    assert run_filter(sc, backend, return_inds=True)["keep_inds"].cpu().tolist() == [0, 2, 4]


def test_points_outside_the_tables_are_dropped(backend):
    """a lidar or frame index outside the pose table keeps nothing and reads nothing (the documented precondition's safety net)"""
    from neuralsim_amd import lidar_filter as lf
    sc, _ = _scene(1000, 5, 5, 3, 70)
    li = sc["li"].clone()
    li[5], li[300], li[999] = 5, -1, 1 << 40
    fi = sc["fi"].clone()
    fi[7], fi[640] = 3, -2
    s2 = dict(sc, li=li, fi=fi)
    got = run_filter(s2, backend, return_inds=True)["keep_inds"].cpu()
    want = run_filter(sc, backend, return_inds=True)["keep_inds"].cpu()
    drop = torch.tensor([5, 300, 999, 7, 640])
    assert torch.equal(got, want[~torch.isin(want, drop)])


# ------------------------------------------------------------------------------------------------ 5. project_pts_in_image
def test_project_pts_in_image(backend):
    from neuralsim_amd import lidar_filter as lf
    base, an0 = _scene(1000, 5, 5, 1, 1)
    pts = an0["q32"]["p"].contiguous()
    pts = pts[torch.isfinite(pts).all(-1)].contiguous()
    N = pts.shape[0]
    for C in (5, 1):
        cams = {k: (v[:, :C] if isinstance(v, torch.Tensor) and v.dim() > 2 else v[:C]) for k, v in base["cams"].items()}
        sc = _points_scene(pts, cams=cams, ignore=base["ignore"][:, :C])
        an = fref.analyse(sc)
        q64, view64, und = an["q64"], an["dec64"]["view"], an["und_pairs"]
        cs = _camera_set(sc, backend)
        ret = lf.project_pts_in_image(_dev(pts.unsqueeze(0), backend), cs, ignore_mask=_dev(sc["ignore"][0], backend))
        assert type(ret).__name__ == "namedtuple_mask_niuvd" and ret._fields == ("mask", "n", "i", "u", "v", "d")
        mask = ret.mask.cpu()
        assert mask.shape == (C, N) and mask.dtype == torch.bool and ret.n == int(mask.sum()) == ret.u.numel()
        assert ret.u.dtype == ret.v.dtype == ret.i.dtype == torch.long and ret.d.dtype == torch.float32
        assert bool((mask == view64)[~und].all())
        # the compaction in nonzero order (camera-major), on the decidable pairs
        gi, gn = mask.nonzero(as_tuple=True)
        assert torch.equal(ret.i.cpu(), gi)
        wi, wn = view64.nonzero(as_tuple=True)
        gd, wd = ~und[gi, gn], ~und[wi, wn]
        assert torch.equal(gi[gd], wi[wd]) and torch.equal(gn[gd], wn[wd])
        u64, v64, d64 = q64["u"][gi, gn], q64["v"][gi, gn], q64["d"][gi, gn]
        m = an["margins"]
        sure_u = gd & ((u64 - u64.round()).abs() > m["u"])
        sure_v = gd & ((v64 - v64.round()).abs() > m["v"])
        assert torch.equal(ret.u.cpu()[sure_u], u64.long()[sure_u]) and torch.equal(ret.v.cpu()[sure_v], v64.long()[sure_v])
        assert float((ret.d.cpu().double() - d64)[gd].abs().max()) <= m["d"]
        # the dense kernel output itself (measured, printed): u, v, d against float64 on the decidable in-view pairs
        dense = [torch.empty([C, N], dtype=torch.float32, device=backend) for _ in range(3)]
        dmask = torch.empty([C, N], dtype=torch.uint8, device=backend)
        _product_lib.call("nsim_cam_project", _dev(pts, backend), N, cs.table, cs.c_models, C, 1e-4, None, 0, 0, dmask, *dense)
        errs = [float((t.cpu().double() - q64[k])[gi, gn][gd].abs().max()) for t, k in zip(dense, "uvd")]
        print(f"cam project C {C}: kernel |u v d - f64| " + " ".join(f"{e:.3e}" for e in errs) + " | margins (2 x the f32 composition) "
              + " ".join(f"{m[k]:.3e}" for k in "uvd") + f" | in-view pairs {int(gd.sum())}, undecidable pairs {int(und.sum())}")
        assert float(und.float().mean()) <= MAX_UNDECIDABLE and int(gd.sum()) > 0.02 * N
        # the filter and the projection share the device function: identical on EVERY point
        out = run_filter(sc, backend, return_inds=True)
        assert torch.equal(_keep_mask(out, N), mask.any(0))
        if C == 1:                       # the single-camera form
            one = lf.CameraSet(_dev(cams["c2w"][0, 0].contiguous(), backend), _dev(cams["intr"][0, 0].contiguous(), backend),
                               cams["hw"][0], cams["models"][0], _dev(cams["dist"][0, 0].contiguous(), backend))
            r1 = lf.project_pts_in_image(_dev(pts, backend), one, ignore_mask=_dev(sc["ignore"][0, 0].contiguous(), backend))
            assert type(r1).__name__ == "namedtuple_mask_nuvd" and r1._fields == ("mask", "n", "u", "v", "d")
            assert torch.equal(r1.mask.cpu(), mask[0]) and r1.n == ret.n
            for a, b in ((r1.u, ret.u), (r1.v, ret.v), (r1.d, ret.d)):
                assert fref.copies_equal(a.cpu(), b.cpu())
    empty = lf.project_pts_in_image(_dev(torch.zeros(0, 3), backend), cs)
    assert empty.mask.shape == (1, 0) and empty.n == 0 and empty.d.shape == (0,)


# ------------------------------------------------------------------------------------------------ 6. bank = frames
def test_bank_equals_the_frames(backend):
    from neuralsim_amd import lidar_filter as lf
    sc, _ = _scene(1000, 5, 5, 3, 70)
    bank = run_filter(sc, backend, return_inds=True, return_pts=True)
    cuts = _frame_cuts(1000, 3)
    off = [int(x) for x in sc["box_offsets"]]
    frames, per = [], []
    for f in range(3):
        sel = slice(cuts[f], cuts[f + 1])
        frames.append(_data(sc, backend, sel))
        per.append(lf.filter_lidar(_data(sc, backend, sel), _dev(sc["l2w"][f].contiguous(), backend), cams=_camera_set(sc, backend, f),
                                   ignore_mask=_dev(sc["ignore"][f].contiguous(), backend), aabb=_dev(sc["aabb"], backend),
                                   boxes=_dev(sc["boxes"][off[f]:off[f + 1]].contiguous(), backend), return_inds=True, return_pts=True))
    fo = bank["frame_offsets"].cpu()
    assert fo.dtype == torch.long and fo.tolist() == [0] + list(np.cumsum([int(p["ranges"].shape[0]) for p in per]))
    assert int(fo[-1]) == bank["ranges"].shape[0] and all(p["ranges"].shape[0] > 0 for p in per)
    for k in ("rays_o", "rays_d", "ranges", "li", "pts_world"):
        assert fref.copies_equal(bank[k].cpu(), torch.cat([p[k].cpu() for p in per])), k
    assert torch.equal(bank["keep_inds"].cpu(), torch.cat([p["keep_inds"].cpu() + cuts[f] for f, p in enumerate(per)]))
    assert torch.equal(bank["frame_inds"].cpu(), torch.repeat_interleave(torch.arange(3), fo[1:] - fo[:-1]))
    # the list-of-frames form (per-frame dicts and box lists) is the same pass
    listed = lf.filter_lidar_bank(frames, _dev(sc["l2w"].contiguous(), backend), cams=_camera_set(sc, backend),
                                  ignore_mask=_dev(sc["ignore"], backend), aabb=_dev(sc["aabb"], backend),
                                  boxes=[_dev(sc["boxes"][off[f]:off[f + 1]].contiguous(), backend) for f in range(3)], return_inds=True)
    for k in ("rays_o", "rays_d", "ranges", "li", "keep_inds", "frame_inds", "frame_offsets"):
        assert fref.copies_equal(listed[k].cpu(), bank[k].cpu()), k


# ------------------------------------------------------------------------------------------------ 7. the reference's frozen outputs
def _fixture_scene(fx):
    cams = dict(c2w=fx["cam_c2w"][:, :3].unsqueeze(0).contiguous(), intr=fx["cam_intr"].unsqueeze(0), hw=fx["cam_hw"],
                models=list(fx["cam_models"]), dist=fx["cam_dist"].unsqueeze(0),
                raw=(fx["cam_intr_raw"], fx["cam_hw_raw"], fx["downscale"]))       # what ``CameraSet`` is given: stored size + downscale
    sc = _points_scene(fx["pts"], ranges=fx["data"]["ranges"], cams=cams, ignore=fx["ignore"].unsqueeze(0), aabb=fx["aabb"],
                       boxes=fx["boxes"], box_offsets=torch.tensor([0, fx["boxes"].shape[0]], dtype=torch.int32), filter_valid=True)
    return sc


def test_frozen_reference_fixture(backend):
    """the reference's own ``MultiCamBundle.project_pts_in_image`` and ``SceneDataLoader._filter_lidar_gts`` (unchanged, on CPU
    attributes; tests/golden/make_lidar_filter_fixture.py) replayed without the reference tree"""
    from neuralsim_amd import lidar_filter as lf
    fx = torch.load(GOLDEN, map_location="cpu", weights_only=True)
    full = _fixture_scene(fx)
    N = fx["pts"].shape[0]
    stages = dict(valid=dict(valid=True, cams=False, aabb=False, objs=False), cams=dict(valid=True, cams=True, aabb=False, objs=False),
                  aabb=dict(valid=True, cams=True, aabb=True, objs=False), objs=dict(valid=True, cams=True, aabb=True, objs=True))
    for name, flags in stages.items():
        sc = _subscene(full, **flags)
        an = fref.analyse(sc)
        und = an["und"]
        assert float(und.float().mean()) <= MAX_UNDECIDABLE
        got = run_filter(sc, backend, return_inds=True)["keep_inds"].cpu()
        want = fx["kept"][name]
        assert torch.equal(got[~und[got]], want[~und[want]]), name
        assert want.numel() > 0.02 * N
    assert fx["kept"]["objs"].numel() < fx["kept"]["aabb"].numel() < fx["kept"]["cams"].numel() < fx["kept"]["valid"].numel() < N
    # the projection tuple
    sc = _subscene(full, valid=False, cams=True, aabb=False, objs=False)
    an = fref.analyse(sc)
    und = an["und_pairs"]
    ret = lf.project_pts_in_image(_dev(fx["pts"].unsqueeze(0).contiguous(), backend), _camera_set(sc, backend),
                                  ignore_mask=_dev(fx["ignore"], backend))
    pj = fx["proj"]
    mask = ret.mask.cpu()
    assert bool((mask == pj["mask"])[~und].all()) and float(und.float().mean()) <= MAX_UNDECIDABLE
    gi, gn = mask.nonzero(as_tuple=True)
    wi, wn = pj["mask"].nonzero(as_tuple=True)
    assert torch.equal(pj["i"], wi) and pj["n"] == wi.numel()
    gd, wd = ~und[gi, gn], ~und[wi, wn]
    assert torch.equal(gi[gd], wi[wd]) and torch.equal(gn[gd], wn[wd])
    m = an["margins"]
    u64, v64 = an["q64"]["u"][wi, wn], an["q64"]["v"][wi, wn]
    su = wd & ((u64 - u64.round()).abs() > m["u"])
    sv = wd & ((v64 - v64.round()).abs() > m["v"])
    gsu, gsv = su[wd], sv[wd]
    assert torch.equal(ret.u.cpu()[gd][gsu], pj["u"][su]) and torch.equal(ret.v.cpu()[gd][gsv], pj["v"][sv])
    assert float((ret.d.cpu()[gd] - pj["d"][wd]).abs().max()) <= m["d"]


# ------------------------------------------------------------------------------------------------ 8. the reference's loader
needs_reference = ref_glue.needs_reference(
    ref_glue.readable(ref_glue.REF_ROOT / "dataio/data_loader/base_loader.py"),
    reason="executes the reference's own sources, which only the authoring machine has (emulator backend); what it pins is "
           "replayed on the GPU box from the reference's frozen outputs: test_frozen_reference_fixture")


@contextlib.contextmanager
def _reference_loader_modules():
    """the reference's scene graph and ``SceneDataLoader``, imported unchanged over the ``nr3d_lib`` shim (with the import-time
    stand-ins of tools/run_reference_train.py for the third-party packages it never calls); everything is removed again on exit"""
    root = Path(__file__).resolve().parent.parent
    saved_path, saved_meta, before = list(sys.path), list(sys.meta_path), set(sys.modules)
    sys.path.insert(0, str(root / "tools"))
    sys.path.append(str(ref_glue.REF_ROOT))
    try:
        import run_reference_train as rrt
        rrt._install_third_party_stubs()
        from app.resources import create_scene_bank
        from dataio.data_loader.base_loader import SceneDataLoader
        yield create_scene_bank, SceneDataLoader
    finally:
        sys.path[:], sys.meta_path[:] = saved_path, saved_meta
        for k in set(sys.modules) - before:
            if k.split(".")[0] in ("app", "dataio", "torch_scatter", "run_reference_train") or type(sys.modules[k]).__name__ == "_Stub":
                del sys.modules[k]


@needs_reference
def test_reference_filter_adapter(backend, tmp_path, monkeypatch):
    """``reference_filter_adapter`` installed as ``SceneDataLoader._filter_lidar_gts`` against the reference's own method, through the
    reference's ``filter_lidar_gts`` on the synthetic street dataset: a single lidar and a merged sweep (``li``), cameras with the
    configured ignore masks, an AABB, object boxes from metas built here (the synthetic scene carries none)"""
    from neuralsim_amd import lidar_filter as lf
    from neuralsim_amd.dataio import SyntheticStreetDataset
    from nr3d_lib.config import ConfigDict
    cam_ids = ["camera_FRONT", "camera_FRONT_LEFT", "camera_FRONT_RIGHT"]
    with _reference_loader_modules() as (create_scene_bank, SceneDataLoader):
        ds = SyntheticStreetDataset(ConfigDict(n_frames=4, image_h=24, image_w=32))
        cfg = ConfigDict(scenarios=["synthetic_street"],
                         observer_cfgs=ConfigDict(Camera=ConfigDict(list=cam_ids), RaysLidar=ConfigDict(list=["lidar_TOP"])),
                         on_load=ConfigDict(no_objects=True, align_orientation=True, consider_distortion=True, scene_graph_has_ego_car=True))
        bank, _ = create_scene_bank(dataset=ds, device=backend, scenebank_cfg=cfg, drawable_class_names=["Street", "Distant", "Sky"],
                                    misc_node_class_names=["node", "EgoVehicle", "EgoDrone"], scenebank_root=str(tmp_path))
        scene = bank[0]
        tags = ConfigDict(camera=ConfigDict(downscale=1, list=cam_ids), image_occupancy_mask=ConfigDict(), image_human_mask=ConfigDict(),
                          image_ignore_mask=ConfigDict(ignore_not_occupied=False, ignore_dynamic=False, ignore_human=True),
                          lidar=ConfigDict(list=["lidar_TOP"], multi_lidar_merge=True))
        loader = SceneDataLoader(bank, ds, config=ConfigDict(preload=False, tags=tags), device=backend, is_master=False)
        frame = 1
        g = torch.Generator().manual_seed(3)
        raw = loader.get_lidar_gts(scene.id, "lidar_TOP", frame, device=backend)
        scene.frozen_at_global_frame(frame)
        hit = scene.observers["lidar_TOP"].world_transform(torch.addcmul(raw["rays_o"], raw["rays_d"], raw["ranges"].unsqueeze(-1)))
        scene.unfrozen()
        hit = hit[raw["ranges"] > 0].cpu()
        rows = []
        for _ in range(5):                                           # boxes at points the beams hit
            m = torch.cat([_rodrigues([0.0, 0.0, 1.0], float(torch.rand(1, generator=g)) * 3), torch.zeros(3, 1, dtype=torch.float64)], 1)
            m[:, 3] = hit[int(torch.randint(0, hit.shape[0], (1,), generator=g))].double()
            rows.append(torch.cat([m.reshape(-1), torch.tensor([6.0, 3.0, 4.0], dtype=torch.float64)]).numpy())
        per_frame = [np.empty([0, 15])] * 4
        per_frame[frame + scene.data_frame_offset] = np.stack(rows)
        scene.metas["obj_box_list_per_frame"] = {"Vehicle": per_frame, "Sign": [np.stack(rows[:1]) * 0 + 1.0] * 4}
        real = SceneDataLoader._filter_lidar_gts
        seen = {}

        def adapter(self, data, pts, frozen_scene, **kw):
            seen.update(pts=pts.detach().cpu().clone(), frozen=frozen_scene)
            cams = [frozen_scene.observers[c] for c in cam_ids]
            seen["cams"] = dict(c2w=torch.stack([c.world_transform.mat_4x4()[:3] for c in cams]).unsqueeze(0).detach().cpu().clone(),
                                intr=torch.stack([c.intr.mat_3x3() for c in cams]).unsqueeze(0).detach().cpu().clone(),
                                hw=torch.stack([torch.stack([c.intr.H, c.intr.W]) for c in cams]).cpu(),
                                models=[type(c.intr).model for c in cams],
                                dist=torch.stack([torch.cat([c.intr.subattr["distortion"].tensor, torch.zeros(5)])[:5]
                                                  for c in cams]).unsqueeze(0).detach().cpu().clone())
            return lf.reference_filter_adapter(self, data, pts, frozen_scene, **kw)
        aabb = torch.tensor([[-30.0, -25.0, -10.0], [35.0, 30.0, 10.0]])
        runs = [("lidar_TOP", dict(filter_in_cams=True)), (["lidar_TOP"], dict(filter_in_cams=True)),
                (["lidar_TOP"], dict(filter_valid=True, filter_in_cams=False, filter_out_objs=True, filter_out_obj_classnames=["Vehicle"])),
                (["lidar_TOP"], dict(filter_in_cams=True, filter_in_aabb=aabb, filter_out_objs=True, filter_out_obj_classnames=["Vehicle"]))]
        for lidar_id, kw in runs:
            raw = (loader.get_lidar_gts(scene.id, lidar_id, frame, device=backend) if isinstance(lidar_id, str)
                   else loader.get_merged_lidar_gts(scene.id, frame, device=backend))
            N = raw["ranges"].shape[0]
            raw["idx"] = torch.arange(N)
            assert ("li" in raw) == (not isinstance(lidar_id, str))
            monkeypatch.setattr(SceneDataLoader, "_filter_lidar_gts", real)
            want = loader.filter_lidar_gts(scene.id, lidar_id, frame, dict(raw), **kw)
            monkeypatch.setattr(SceneDataLoader, "_filter_lidar_gts", adapter)
            got = loader.filter_lidar_gts(scene.id, lidar_id, frame, dict(raw), **kw)
            assert list(got.keys()) == list(want.keys()) == list(raw.keys())
            assert scene.i is None                                   # the reference's method unfroze the scene again
            sc = _points_scene(seen["pts"], ranges=raw["ranges"].cpu(), filter_valid=kw.get("filter_valid", True))
            if kw.get("filter_in_cams"):
                sc["cams"] = seen["cams"]
                masks = [loader.get_image_ignore_mask(scene_id=scene.id, cam_id=c, frame_ind=frame, device=backend) for c in cam_ids]
                sc["ignore"] = torch.stack(masks).unsqueeze(0).cpu()
            if "filter_in_aabb" in kw:
                sc["aabb"] = aabb
            if kw.get("filter_out_objs"):
                sc["boxes"], sc["box_offsets"] = torch.tensor(np.stack(rows), dtype=torch.float), torch.tensor([0, 5], dtype=torch.int32)
            an = fref.analyse(sc)
            und = an["und"]
            gi, wi = got["idx"].cpu(), want["idx"].cpu()
            print(f"adapter {lidar_id} {sorted(kw)}: kept {gi.numel()} of {N} (reference {wi.numel()}), undecidable {int(und.sum())}")
            assert torch.equal(gi[~und[gi]], wi[~und[wi]]) and torch.equal(wi[~und[wi]], an["dec64"]["keep"].nonzero()[:, 0][~und[an["dec64"]["keep"]]])
            assert 0 < wi.numel() < N and float(und.float().mean()) <= MAX_UNDECIDABLE
            for k in raw:
                assert fref.copies_equal(got[k].cpu(), raw[k].cpu()[gi]), k


# ------------------------------------------------------------------------------------------------ 9. trainer hook
def test_street_trainer_takes_a_filtered_bank(backend):
    from neuralsim_amd import scenarios as sc
    torch.manual_seed(1234)
    tr = sc.build_street_trainer(backend, small=True, rays_per_gpu=48, lidar_rays=48, num_uniform=16,
                                 lidar_filter_kwargs=dict(filter_in_cams=True))
    L = tr.lidar
    assert L["ranges"].dim() == 2 and L["ranges"].shape[0] == 1 and L["rays_o"].shape == (1, L["ranges"].shape[1], 3)
    world = sc.street_world()
    o, d, r = sc.street_lidar(world, n_ego=2, beams=512)
    T = L["ranges"].shape[1]
    assert 0 < T < int((r > 0).sum())                                     # a strict subset of the valid beams
    rows = torch.cat([o.reshape(-1, 3), d.reshape(-1, 3), r.reshape(-1, 1)], dim=1)
    got = torch.cat([L["rays_o"][0], L["rays_d"][0], L["ranges"][0, :, None]], dim=1).cpu()
    pos = {row.numpy().tobytes(): k for k, row in enumerate(rows)}
    src = torch.tensor([pos[row.numpy().tobytes()] for row in got])       # every kept beam is an input beam, bit for bit ...
    assert bool((src[1:] > src[:-1]).all())                               # ... in the input order
    # every kept return is in view of a camera of its own ego pose (float64; a margin of a thousandth of a pixel)
    intr, c2w, WH = sc.street_rig(n_ego=2, H=24, W=24, f=0.625 * 24)
    p = (got[:, :3] + got[:, 3:6] * got[:, 6:7]).double()
    frame = src // 512
    seen = torch.zeros(T, dtype=torch.bool)
    for v in range(c2w.shape[0]):
        cam = ((p - c2w[v, :3, 3].double()).unsqueeze(-2) * c2w[v, :3, :3].double().T).sum(-1)
        u = intr[v, 0, 0].double() * cam[:, 0] / cam[:, 2] + intr[v, 0, 2].double()
        w = intr[v, 1, 1].double() * cam[:, 1] / cam[:, 2] + intr[v, 1, 2].double()
        seen |= (frame == v // 6) & (cam[:, 2] > 1e-4 - 1e-6) & (u > -1e-3) & (u < 24 + 1e-3) & (w > -1e-3) & (w < 24 + 1e-3)
    assert bool(seen.all())
    loss = tr.train_step_lidar(0)
    assert math.isfinite(float(loss))


# ------------------------------------------------------------------------------------------------ 10. refusals
def test_refusals(backend, monkeypatch):
    from neuralsim_amd import lidar_filter as lf
    sc, _ = _scene(63, 5, 5, 1, 1)
    data = _data(sc, backend)
    l2w = _dev(sc["l2w"][0].contiguous(), backend)
    cams = _camera_set(sc, backend)
    with pytest.raises(ValueError, match="unknown camera model"):
        lf.CameraSet(_dev(sc["cams"]["c2w"][0].contiguous(), backend), _dev(sc["cams"]["intr"][0].contiguous(), backend), sc["cams"]["hw"],
                     ["pinhole", "opencv", "fisheye", "opencv", "equirect"])
    with pytest.raises(ValueError, match="l2w must be contiguous"):
        lf.filter_lidar(data, _dev(sc["l2w"][0].transpose(-1, -2).contiguous(), backend).transpose(-1, -2)[:, :, :])
    with pytest.raises(ValueError, match="l2w must be"):
        lf.filter_lidar(data, l2w[:, :2])
    one = {k: v for k, v in data.items() if k != "li"}
    with pytest.raises(ValueError, match="single pose"):
        lf.filter_lidar(data, l2w[0].contiguous())
    with pytest.raises(ValueError, match="smaller than the largest image"):
        lf.filter_lidar(data, l2w, cams=cams, ignore_mask=_dev(torch.zeros(5, 60, 96, dtype=torch.bool), backend))
    with pytest.raises(ValueError, match="ignore_mask must be"):
        lf.filter_lidar(data, l2w, cams=cams, ignore_mask=_dev(torch.zeros(4, 64, 96, dtype=torch.bool), backend))
    with pytest.raises(ValueError, match="rays_d must be"):
        lf.filter_lidar(dict(data, rays_d=data["rays_d"][:-1].contiguous()), l2w)
    with pytest.raises(ValueError, match="rays_o must be contiguous"):
        lf.filter_lidar(dict(one, rays_o=_dev(torch.zeros(3, 63), backend).t()), l2w[0].contiguous())
    with pytest.raises(ValueError, match="must be a tensor with 63 rows"):
        lf.filter_lidar(dict(one, intensity=_dev(torch.zeros(62), backend)), l2w[0].contiguous())
    with pytest.raises(ValueError, match="boxes must be"):
        lf.filter_lidar(data, l2w, boxes=_dev(torch.zeros(3, 12), backend))
    with pytest.raises(ValueError, match="aabb must be"):
        lf.filter_lidar(data, l2w, aabb=_dev(torch.zeros(3, 2), backend))
    with pytest.raises(ValueError, match="belongs to filter_lidar_bank"):
        lf.filter_lidar(data, l2w, frame_inds=_dev(torch.zeros(63, dtype=torch.long), backend))
    with pytest.raises(ValueError, match="needs frame_inds"):
        lf.filter_lidar_bank(data, _dev(sc["l2w"].contiguous(), backend))
    with pytest.raises(ValueError, match="takes the cameras of one frame"):
        s3, _ = _scene(257, 1, 1, 3, 70)
        lf.project_pts_in_image(_dev(torch.zeros(4, 3), backend), _camera_set(s3, backend))
    # the C entry points: sizes, pointers and model ids
    lib = _product_lib.get_lib()
    import ctypes
    bad = (ctypes.c_int32 * 1)(3)
    good = (ctypes.c_int32 * 1)(1)
    assert lib.nsim_cam_project(None, 4, None, bad, 1, 1e-4, None, 0, 0, None, None, None, None, None) == 62          # model id
    assert lib.nsim_cam_project(None, 1 << 31, None, good, 1, 1e-4, None, 0, 0, None, None, None, None, None) == 62   # N
    assert lib.nsim_cam_project(None, -1, None, good, 1, 1e-4, None, 0, 0, None, None, None, None, None) == 2
    assert lib.nsim_cam_project(None, 4, None, good, 1, 1e-4, None, 0, 0, None, None, None, None, None) == 4          # outputs
    assert lib.nsim_cam_project(None, 0, None, None, 0, 1e-4, None, 0, 0, None, None, None, None, None) == 0          # no launch
    assert lib.nsim_cam_project(None, 4, None, None, 33, 1e-4, None, 0, 0, None, None, None, None, None) == 62
    cnt_args = lambda N, C, m, B: (None, None, None, None, None, N, None, 1, 1, 1, None, m, C, 1e-4, None, 0, 0, None, None, None, B,
                                   None, None, None)
    assert lib.nsim_lidar_filter_count(*cnt_args(0, 0, None, 0)) == 0
    assert lib.nsim_lidar_filter_count(*cnt_args(-1, 0, None, 0)) == 2
    assert lib.nsim_lidar_filter_count(*cnt_args(4, 0, None, -1)) == 2
    assert lib.nsim_lidar_filter_count(*cnt_args(1 << 31, 0, None, 0)) == 62
    assert lib.nsim_lidar_filter_count(*cnt_args(4, 1, bad, 0)) == 62
    assert lib.nsim_lidar_filter_count(*cnt_args(4, 0, None, 0)) == 4
    emit_args = lambda N: (None,) * 7 + (N, None, 1, 1) + (None,) * 8
    assert lib.nsim_lidar_filter_emit(*emit_args(0)) == 0 and lib.nsim_lidar_filter_emit(*emit_args(-1)) == 2
    assert lib.nsim_lidar_filter_emit(*emit_args(1 << 31)) == 62 and lib.nsim_lidar_filter_emit(*emit_args(4)) == 4
    assert b"lidar filter" in lib.nsim_strerror(62)
    # host tensors: the product's own check (the emulator backend patches it away) refuses them by name
    monkeypatch.setattr(_product_lib, "require_device", _REQUIRE_DEVICE)
    cpu = {k: v.cpu() for k, v in data.items()}
    with pytest.raises(RuntimeError, match="ranges must live on a HIP device.*no CPU path"):
        lf.filter_lidar(cpu, l2w)
    if backend.type == "cuda":           # (on the emulator every tensor is a host tensor: the first one checked is refused)
        with pytest.raises(RuntimeError, match="l2w must live on a HIP device"):
            lf.filter_lidar(data, l2w.cpu())
    with pytest.raises(RuntimeError, match="pts must live on a HIP device"):
        lf.project_pts_in_image(torch.zeros(4, 3), cams)
    with pytest.raises(RuntimeError, match="c2w must live on a HIP device"):
        lf.CameraSet(torch.eye(4), torch.eye(3), (4, 4))
