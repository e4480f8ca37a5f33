"""The table gathers, entry point by entry point, against float64 (tests/gather_ref.py): ``nsim_lotd_fwd`` (out, dydx),
``nsim_lotd_gather_lm`` (f16x2 * 1024 and f32x2 planes), ``nsim_field_fwd`` with ``wpack == NULL`` (h + dh/dx planes, f32 and
f16), ``nsim_lotd_hess_dx``, ``nsim_permuto_gather`` (feature planes, h + dh/dx planes, with and without a condition) and the
4-D gather inside ``nsim_distant_fwd`` (h_planes only).  Tables and planes are built here: no decoder output is compared.

What is pinned per entry point: every (level, valid point, feature) within the bound below; with NaN-poisoned planes, every
row the contract names written exactly where it says and NOTHING else (points past the valid count, the pitch padding and the
rows past the dealt ones are still NaN); masked levels exactly zero without a table read; the bit-identities the code claims.

Rows past the pyramid -- LoTD (no-grad and with-grad) and the permutohedral gather: ZEROS in rows num_levels .. 15 (<= 16 levels)
or up to the next multiple of 8 (17..32 levels), untouched beyond.  That is what ``deal_levels`` / ``permuto_launch_fwd`` do
and what the 16-level decoders rely on (they read all 16 rows against zero weight columns); the sentence "levels past
num_levels are not written" of include/nsim.h describes the rows beyond those only.  The 4-D gather writes the pyramid's own
rows at pitch S and leaves rows num_levels .. 15 untouched: the distant decoders guard every row by num_levels.

Bound (derived, not measured -- gather_ref.py):  |got - ref| <= (r_l + 16) 2^-24 W A per (level, point, feature), r_l = 9 R_l
(12 R_l in 4-D, (in_dim + 1) x the largest scale on the lattice); x dscale_a for d feature / d x_a; an f16 output adds its half
ulp.  Features are continuous across cell faces and are compared at EVERY (level, point) of every set.  d features / d x and the
hess term are one-sided at a face: the margin-keeping sets of scatter_ref.py are compared whole (margin asserted), the lattice
set too (``pos`` is exact there, floor / "top face -> last cell" is a definite answer), and on the whole-box set and the deep
pyramids -- where no origin keeps 1e-3 from every face of a 2048-vertex level -- the (level, point) pairs nearer than 1e-3 to a
cell decision are left out of the DERIVATIVE comparison only (still finite; the dyadic half of the whole-box set sits ON decisions).

Worst observed error / bound over all cases of this file (every case prints its own as ``RATIO <entry point> <device> <value>``):

    entry point                     emulator    MI355X
    nsim_lotd_fwd                   0.0750      0.0750
    nsim_lotd_gather_lm             0.0688      0.0688
    nsim_lotd_gather_lm/f16         0.9440      0.9440
    nsim_field_fwd(gather)          0.1031      0.1031
    nsim_field_fwd(gather)/f16      0.9667      0.9667
    nsim_lotd_hess_dx               0.0721      0.0721
    nsim_permuto_gather             0.1034      0.1034
    nsim_permuto_gather/f16         0.9646      0.9646
    nsim_distant_fwd(gather)        0.0088      0.0088

(``/f16``: the f16 outputs -- feature planes f16(sat(1024 f)), dh/dx planes f16(sat(J)).  Their bound is the f32 one plus half an
f16 ulp, and a rounding attains its half ulp: a ratio near 1 is the conversion itself, not the gather; the f32 value under it is
pinned by the f32 rows of the table and by the bit-identity f16 plane == f16(sat(1024 x f32 plane)).  The library is compiled
with -ffp-contract=off, as the emulator: a gather has no atomics, so the two backends give the same bits.)

``nsim_lotd_fwd`` enumerates the vertices as the no-grad level-major form does (``corner = slot ^ mask``) and is bit-identical
to the f32 planes on the unit box; the with-grad form goes through the per-axis operand tables and is bit-identical too.

Known limit, not exercised: the table offsets are 32-bit (``off + goff + 2 idx``) -- a flat batched table beyond 2^32 fp16
elements cannot be built at test size.
"""
import functools
import os

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings, strategies as st

import gather_ref as gr
import scatter_ref as sr
from oracle import distant as odist, lotd as olotd, permuto as operm
from neuralsim_amd import _lib
from neuralsim_amd.grid_encodings.lotd import LoTDConfig
from neuralsim_amd.grid_encodings.permuto import PermutoConfig

_N = int(os.environ.get("NSIM_FUZZ_EXAMPLES", "0"))
SET = dict(max_examples=_N or 12, derandomize=_N == 0, deadline=None,
           suppress_health_check=[HealthCheck.function_scoped_fixture])

F64 = torch.float64
COUNTS = [1, 63, 64, 65, 127, 128, 129, 192, 257, 385]
# scatter_ref's pyramid (T = 2^9: 3, 5, 8 dense, 9 and finer hashed) continued to 32 levels
RES32 = [3, 5, 8, 9, 11, 17, 33, 67, 129, 257, 300, 384, 450, 513, 600, 700, 800, 900, 1025, 1100, 1200, 1300, 1400, 1500, 1600,
         1700, 1800, 1900, 2000, 2048, 2049, 2048]
CUBOID_BOX = ([-1.0, -1.5, -2.0], [1.0, 1.5, 2.0])


def _sync(device):
    if device.type == "cuda":
        torch.cuda.synchronize()


def _dv(t, device):
    return None if t is None else t.to(device).contiguous()


def _dev_name(device):
    return "hip" if device.type == "cuda" else "emu"


# ------------------------------------------------------------------------------------------------- pyramids, tables, sets
@functools.lru_cache(maxsize=None)
def _lotd(kind="generic", L=10):
    if kind == "generic":
        cfg = LoTDConfig(RES32[:L], 2, 9)
    elif kind == "lattice":
        cfg = LoTDConfig(sr.LATTICE_RES, 2, 8)
    elif kind == "tiny":
        cfg = LoTDConfig([2, 3, 5, 9, 17, 33], 2, 4)
    elif kind == "cuboid":
        cfg = LoTDConfig([[3, 4, 5], [5, 7, 9], [9, 13, 17], [17, 25, 33], [40, 60, 80]], 2, 9)
        cfg.set_aabb([[-1.0, -1.5, -2.0], [1.0, 1.5, 2.0]])
    return cfg, sr.lotd_levels(cfg)


def _fresh_lotd(kind="generic", L=10):
    """a config of its own for the tests that change the meta (n_active_levels)"""
    return _lotd.__wrapped__(kind, L)


def _table(n, seed=3, amp=0.5):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(n, generator=g) * 2 - 1) * amp).half()


def _box_of(kind):
    return CUBOID_BOX if kind == "cuboid" else (-1.0, 1.0)


@functools.lru_cache(maxsize=None)
def _margin_set(name, kind="generic"):
    """scatter_ref's margin-keeping sets on the 10-level pyramid: neighbouring lanes in neighbouring cells"""
    lv = _lotd(kind)[1]
    kw = dict(margin_fn=sr.lotd_margin(lv), box=_box_of(kind))
    if name.startswith("ray"):
        return sr.dense_ray(int(name[3:]), **kw)
    if name.startswith("interleaved"):
        return sr.interleaved(int(name[11:]), **kw)
    if name == "batched":
        return sr.batched_pair(200, margin_fn=sr.lotd_margin(lv))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _box_set(n, kind="generic"):
    return gr.whole_box(n, box=_box_of(kind))


def _get_set(name, kind="generic"):
    if name == "lattice":
        return sr.lattice_points()
    if name.startswith("box"):
        return _box_set(int(name[3:]), kind)
    return _margin_set(name, kind)


def _pair_margin(lv, p):
    """[L, S]: distance of pos from the nearest cell decision -- an integer 1 .. R - 2 (the clamp makes 0 and R - 1 none)"""
    out = []
    for l in range(lv.num_levels):
        pos, R3 = sr._lotd_pos(lv, p, l)
        near = torch.minimum(torch.maximum(pos.round(), torch.ones(3, dtype=F64)), R3 - 2.0)
        d = (pos - near).abs()
        d = torch.where((R3 > 2.0).expand_as(d), d, torch.full_like(d, float("inf")))
        out.append(d.amin(-1))
    return torch.stack(out)


def _jmask(lv, sset, form, name):
    """(level, point) pairs whose derivative is compared.  Margin-keeping sets: all (the margin is asserted); the lattice set:
    all (pos exact, asserted by test_lattice_is_exact); else the pairs at least MARGIN from a decision."""
    L, S = lv.num_levels, sset.S
    if name == "lattice":
        return torch.ones(L, S, dtype=torch.bool)
    if not name.startswith("box"):
        m = min(sr.lotd_margin(lv)(sset, "rays"), sr.lotd_margin(lv)(sset, "x"))
        assert m >= sr.MARGIN, f"{sset.name}: decision margin {m}"
        return torch.ones(L, S, dtype=torch.bool)
    mask = _pair_margin(lv, sset.points(form)) >= sr.MARGIN
    # (up to half of a whole-box set are dyadic points, ON a decision of every level whose R - 1 their denominator divides; a
    # uniform point is within 1e-3 of one with probability ~ 3 x 2e-3)
    assert float(mask.double().mean()) >= 0.45 or S < 8
    return mask


def _pt_args(sset, form, device, need_ridx=False):
    if form == "x":
        return _dv(sset.x32(), device), None, None, None, (_dv(sset.ridx, device) if need_ridx else None)
    return None, _dv(sset.o, device), _dv(sset.d, device), _dv(sset.t, device), _dv(sset.ridx, device)


def _fm(cfg, precision):
    fm = _lib.FieldMeta()
    fm.lotd = cfg.meta
    fm.sdf_D, fm.precision, fm.softplus_beta, fm.embed_E = 1, precision, 100.0, 0
    return fm


def _nlp(L):
    return 16 if L <= 16 else 32


def _rows_zeroed(L):
    """rows the LoTD and permutohedral level-major gathers write: the pyramid's, then zeros up to here"""
    return 16 if L <= 16 else (L + 7) & ~7


def _n_dev(n_valid, n_add, device):
    return None if n_valid is None else torch.tensor([n_valid - n_add], dtype=torch.long, device=device)


# ------------------------------------------------------------------------------------------------- the entry points
def _run_lotd_fwd(device, cfg, table, sset, dydx=True):
    S, L = sset.S, cfg.num_levels
    out = torch.empty(S, 2 * L, dtype=torch.float32, device=device)
    jac = torch.empty(S, 2 * L, 3, dtype=torch.float32, device=device) if dydx else None
    _lib.call("nsim_lotd_fwd", _lib.ptr(_dv(sset.x32(), device)), _lib.ptr(_dv(table, device)), cfg.meta, S, _lib.ptr(out),
              _lib.ptr(jac))
    _sync(device)
    return out.cpu().view(S, L, 2).permute(1, 0, 2), (jac.cpu().view(S, L, 2, 3).permute(1, 0, 2, 3) if dydx else None)


def _run_gather_lm(device, cfg, table, sset, form, prec, goff=None, n_valid=None, n_add=3):
    S, L = sset.S, cfg.num_levels
    planes = torch.empty(_nlp(L), _lib.plane_pitch(S), 2, dtype=torch.float16 if prec == 0 else torch.float32, device=device)
    x, o, d, t, ridx = _pt_args(sset, form, device, goff is not None)
    _lib.call("nsim_lotd_gather_lm", _fm(cfg, prec), _lib.ptr(_dv(table, device)), _lib.ptr(x), _lib.ptr(o), _lib.ptr(d),
              _lib.ptr(t), _lib.ptr(ridx), _lib.ptr(_dv(goff, device)), S, _lib.ptr(_n_dev(n_valid, n_add, device)),
              n_add if n_valid is not None else 0, _lib.ptr(planes))
    _sync(device)
    return planes.cpu()


def _run_field_gather(device, cfg, table, sset, form, prec, goff=None, n_valid=None, n_add=3):
    """nsim_field_fwd with wpack == NULL -> (h_planes [NLP, P, 2] f32, J_planes [NLP, P, 2, 3] f16 | f32)"""
    S, L = sset.S, cfg.num_levels
    fm = _fm(cfg, prec)
    jdt = _lib.jplane_dtype(fm)
    assert jdt == (torch.float16 if prec == 0 else torch.float32)
    P = _lib.plane_pitch(S)
    h = torch.empty(_nlp(L), P, 2, dtype=torch.float32, device=device)
    J = torch.empty(_nlp(L), P, 2, 3, dtype=jdt, device=device)
    x, o, d, t, ridx = _pt_args(sset, form, device, goff is not None)
    _lib.call("nsim_field_fwd", fm, _lib.ptr(_dv(table, device)), None, _lib.ptr(x), _lib.ptr(o), _lib.ptr(d), _lib.ptr(t),
              _lib.ptr(ridx), _lib.ptr(_dv(goff, device)), None, S, None, None, None, _lib.ptr(h), _lib.ptr(J),
              _lib.ptr(_n_dev(n_valid, n_add, device)), n_add if n_valid is not None else 0)
    _sync(device)
    return h.cpu(), J.cpu()


def _run_hess(device, cfg, table, sset, form, g, gn, dx0, goff=None):
    x, o, d, t, ridx = _pt_args(sset, form, device, goff is not None)
    dx = _dv(dx0.clone(), device)
    _lib.call("nsim_lotd_hess_dx", cfg.meta, _lib.ptr(_dv(table, device)), _lib.ptr(x), _lib.ptr(o), _lib.ptr(d), _lib.ptr(t),
              _lib.ptr(ridx), _lib.ptr(_dv(goff, device)), sset.S, _lib.ptr(_dv(g, device)), _lib.ptr(_dv(gn, device)), _lib.ptr(dx))
    _sync(device)
    return dx.cpu()


# ------------------------------------------------------------------------------------------------- the comparison
def _accept_rows(name, device, got, ref, bnd, Sv, rows_zero, mask=None):
    """got [NLP, P, ...] (any float dtype, in the reference's units); ref, bnd [L, S, ...] f64.  Rows < L, points < Sv: finite and
    within the bound (``mask`` [L, S]: where compared; finite everywhere); rows L .. rows_zero - 1, points < Sv: exactly 0;
    every other element -- points >= Sv, the pitch padding, rows >= rows_zero -- still NaN.  -> worst error / bound"""
    got = got.double()
    L = ref.shape[0]
    live = got[:L, :Sv]
    assert bool(torch.isfinite(live).all()), f"{name}: a (level, valid point) was not written (or is not finite)"
    err, b = (live - ref[:, :Sv]).abs(), bnd[:, :Sv]
    if mask is not None:
        err, b = err[mask[:, :Sv]], b[mask[:, :Sv]]
    worst = gr.ratio(err, b)
    print(f"RATIO {name} {_dev_name(device)} {worst:.4f}")
    assert bool((got[L:rows_zero, :Sv] == 0.0).all()), f"{name}: rows past the pyramid are not zero"
    assert bool(got[:rows_zero, Sv:].isnan().all()), f"{name}: written at s >= the valid count"
    assert bool(got[rows_zero:].isnan().all()), f"{name}: a row past the dealt ones was written"
    assert worst <= 1.0, f"{name}: worst error / bound = {worst}"
    return worst


def _accept_f16_feat(name, device, planes, ref: gr.GatherRef, Sv, rows_zero):
    """precision-0 feature planes: f16(sat(1024 f))"""
    fb = ref.feat_bound()
    want = gr.f16_sat(ref.feat, gr.H_SCALE)
    assert not bool(torch.isinf(planes[:ref.feat.shape[0], :Sv]).any())
    return _accept_rows(name + "/f16", device, planes.double() / gr.H_SCALE, want, fb + gr.f16_term(want, fb, gr.H_SCALE), Sv, rows_zero)


def _accept_J(name, device, J, ref: gr.GatherRef, Sv, rows_zero, mask):
    jb = ref.J_bound()
    if J.dtype == torch.float16:
        want = gr.f16_sat(ref.J)
        assert not bool(torch.isinf(J[:ref.J.shape[0], :Sv]).any())
        return _accept_rows(name + "/f16", device, J, want, jb + gr.f16_term(want, jb), Sv, rows_zero, mask)
    return _accept_rows(name, device, J, ref.J, jb, Sv, rows_zero, mask)


def _f16_of_f32_planes(p32):
    """what the code says a precision-0 plane is, from the f32 plane of the same launch arguments"""
    return (p32 * gr.H_SCALE).clamp(-gr.F16_MAX, gr.F16_MAX).half()


def _same_bits(a, b):
    if a.dtype == torch.float16:
        return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# =================================================================================================== the reference itself
def test_reference_equals_oracle():
    """gather_ref's f64 features are oracle/lotd.py, oracle/distant.py::lotd4_forward and oracle/permuto.py evaluated in f64; J and
    the hess term are autograd through them (off the lattice: a margin-keeping set)"""
    cfg, lv = _lotd()
    sset = _margin_set("ray64")
    S, L = sset.S, lv.num_levels
    table = _table(cfg.n_params)
    p = sset.points("x")
    ref = gr.lotd_ref(lv, table, p)
    spec = olotd.make_lotd_spec(RES32[:10], 2, 9)
    x = p.clone().requires_grad_(True)
    h = olotd.lotd_forward(x, table.double(), spec)                                   # [S, 2 L]
    tol = 1e-12
    assert (h.detach().view(S, L, 2).permute(1, 0, 2) - ref.feat).abs().max() <= tol
    for k in range(2 * L):
        jk, = torch.autograd.grad(h[:, k].sum(), x, retain_graph=True)
        assert (jk - ref.J[k // 2, :, k % 2]).abs().max() <= tol * float(ref.dsc.max())
    gen = torch.Generator().manual_seed(1)
    g, gn, dx0 = torch.randn(L, S, 2, generator=gen).double(), torch.randn(S, 3, generator=gen).double(), torch.zeros(S, 3, dtype=F64)
    nab, = torch.autograd.grad((h * g.permute(1, 0, 2).reshape(S, 2 * L)).sum(), x, create_graph=True)
    hx, = torch.autograd.grad((nab * gn).sum(), x)
    val, bnd = gr.hess_dx(ref, g, gn, dx0)
    assert (hx - val).abs().max() <= tol * float(val.abs().max()) and bool((bnd > 0).all())
    # the cuboid pyramid over its AABB (the oracle divides by the extent in f64, the meta holds the f32 reciprocal)
    ccfg, clv = _lotd("cuboid")
    cs = _margin_set("ray64", "cuboid")
    cspec = olotd.make_lotd_spec(ccfg.lod_res, 2, 9)
    cspec.aabb = [[-1.0, -1.5, -2.0], [1.0, 1.5, 2.0]]
    ctab = _table(ccfg.n_params)
    hc = olotd.lotd_forward(cs.points("x"), ctab.double(), cspec)
    rc = gr.lotd_ref(clv, ctab, cs.points("x"))
    assert (hc.view(cs.S, -1, 2).permute(1, 0, 2) - rc.feat).abs().max() <= 1e-5          # 1/3 in f32 against 1/3 in f64
    # 4-D
    spec4, _ = _lotd4()
    u = gr.whole_box(129, dim=4, box=(0.0, 1.0)).points("x")
    t4 = _table(spec4.n_params)
    h4 = odist.lotd4_forward(u, t4, spec4)
    assert h4.dtype == F64
    r4 = gr.lotd4_ref(spec4, t4, u)
    assert (h4.view(129, -1, 2).permute(1, 0, 2) - r4.feat).abs().max() <= tol * 4
    # permutohedral
    for D in (3, 5):
        pc, pm = _permuto(D)
        sp = _permuto_set("ray64", D)
        pp = _permuto_points(sp, "x", D)
        tp = _table(pc.n_params)
        ospec = operm.PermutoSpec(D, list(pc.res), 2, pm.T, pm.shift.float())
        ospec.scale_factors = lambda l, pm=pm: pm.scale[l]                            # the meta's f32 values
        xp = pp.clone().requires_grad_(True)
        hp = operm.permuto_forward(xp, tp.double(), ospec)
        rp = gr.permuto_ref(pm, tp, pp)
        assert (hp.detach().view(sp.S, -1, 2).permute(1, 0, 2) - rp.feat).abs().max() <= tol
        for k in range(2 * pm.num_levels):
            jk, = torch.autograd.grad(hp[:, k].sum(), xp, retain_graph=True)
            assert (jk[:, :3] - rp.J[k // 2, :, k % 2]).abs().max() <= 1e-10 * float(pm.scale.max())


def test_comparison_rejects_one_wrong_corner_and_a_wrong_dscale():
    """CPU only: the bound is tight enough for the errors the decoder tolerances hide -- the vertices of ONE of ten levels taken
    from the neighbouring table entry, and R for R - 1 in dscale of one level (while f32 rounding of the reference passes)"""
    cfg, lv = _lotd()
    sset = _margin_set("ray200")
    table = _table(cfg.n_params)
    ref = gr.lotd_ref(lv, table, sset.points("x"))
    fb, jb = ref.feat_bound(), ref.J_bound()
    assert gr.ratio((ref.feat.float().double() - ref.feat).abs(), fb) <= 1.0
    wrong = table.clone()
    wrong[lv.offsets[7]:lv.offsets[7] + 2 * lv.sizes[7]] = table[lv.offsets[7]:lv.offsets[7] + 2 * lv.sizes[7]].roll(2)
    assert gr.ratio((gr.lotd_ref(lv, wrong, sset.points("x")).feat - ref.feat).abs(), fb) > 1.0
    Jw = ref.J.clone()
    Jw[9] *= lv.res3[9][0] / (lv.res3[9][0] - 1.0)
    assert gr.ratio((Jw - ref.J).abs(), jb) > 1.0


def test_lattice_is_exact():
    """on the lattice set the f32 evaluation of pos IS the f64 one, in both forms, and points sit on w = 0 and on the top face"""
    lv = _lotd("lattice")[1]
    sset = sr.lattice_points()
    for form in ("x", "rays"):
        for l in range(lv.num_levels):
            pos32 = (sset.x32() * 0.5 + 0.5) * float(lv.res3[l][0] - 1)
            assert torch.equal(pos32.double(), (sset.points(form) * 0.5 + 0.5) * (lv.res3[l][0] - 1.0))
            assert bool((pos32 == pos32.round()).any()) and bool((pos32 == lv.res3[l][0] - 1.0).any())


# =================================================================================================== the level dealing
def _deal(types, sizes, num_levels, four_d=False):
    """field.hip deal_levels / nerf_field.hip deal_levels4 restated (f32 arithmetic) -> per XCD group a list of (level, half).
    Used ONLY to assert that the pyramids of this file contain the cases; no value check depends on it."""
    f = np.float32
    NL = num_levels if four_d else _rows_zeroed(num_levels)
    cost = [f(0.05 if NL > 16 else 0.35) if l >= num_levels else f(1.0 if types[l] == "Hash" else 0.35) for l in range(NL)]
    size = [sizes[l] if l < num_levels else 0 for l in range(NL)]
    total = f(0)
    for c in cost:
        total = f(total + c)
    limit = f(f(total / f(8.0)) * f(1.08))
    load, groups, used = [f(0)] * 8, [[] for _ in range(8)], [False] * NL
    least = lambda: min(range(8), key=lambda xc: (load[xc], xc))
    for _ in range(NL):
        best = -1
        for l in range(NL):
            if not used[l] and (best < 0 or cost[l] > cost[best] or (cost[l] == cost[best] and size[l] > size[best])):
                best = l
        used[best] = True
        x0 = least()
        if f(load[x0] + cost[best]) <= limit or load[x0] == 0:
            groups[x0].append((best, 0))
            load[x0] = f(load[x0] + cost[best])
        else:
            for half in (1, 2):
                xc = least()
                groups[xc].append((best, half))
                load[xc] = f(load[xc] + f(f(0.5) * cost[best]))
    return groups


def test_pyramids_contain_split_and_whole_levels():
    seen = set()
    for L in (5, 8, 10, 11, 16, 17, 19, 24, 32):
        lv = _lotd("generic", L)[1]
        groups = _deal(lv.types, lv.sizes, L)
        flat = [e for grp in groups for e in grp]
        assert sorted(l for l, h in flat if h != 2) == list(range(_rows_zeroed(L)))          # every dealt row once (or as two halves)
        assert sorted(l for l, h in flat if h == 1) == sorted(l for l, h in flat if h == 2)
        if any(h == 1 for _, h in flat):
            seen.add("split")
        if any(h == 0 for l, h in flat if l < L):
            seen.add("whole")
        if any(len(grp) > 1 for grp in groups):
            seen.add("several")
        if any(h != 0 and l < L and lv.types[l] == "Hash" for l, h in flat):
            seen.add("split-hash")
            seen.add(f"split-hash{L}")
    assert seen >= {"split", "whole", "several", "split-hash", "split-hash16"}, seen
    spec4, _ = _lotd4(12)
    g4 = _deal(spec4.types, spec4.sizes, spec4.num_levels, four_d=True)
    f4 = [e for grp in g4 for e in grp]
    assert any(h == 1 for _, h in f4) and any(h == 0 for _, h in f4), f4


# =================================================================================================== a. nsim_lotd_fwd
@pytest.mark.parametrize("name,kind", [("ray200", "generic"), ("interleaved128", "generic"), ("box257", "generic"),
                                       ("lattice", "lattice"), ("box129", "cuboid"), ("ray200", "cuboid"), ("box129", "tiny")])
def test_lotd_fwd(backend, name, kind):
    """out and dydx: all features, all three derivative components; bit-identical to the level-major f32 planes"""
    cfg, lv = _lotd(kind)
    sset = _get_set(name, kind)
    S, L = sset.S, lv.num_levels
    table = _table(cfg.n_params)
    ref = gr.lotd_ref(lv, table, sset.points("x"))
    out, jac = _run_lotd_fwd(backend, cfg, table, sset)
    _accept_rows("nsim_lotd_fwd", backend, out, ref.feat, ref.feat_bound(), S, L)
    _accept_rows("nsim_lotd_fwd", backend, jac, ref.J, ref.J_bound(), S, L, _jmask(lv, sset, "x", name))
    out_only, _ = _run_lotd_fwd(backend, cfg, table, sset, dydx=False)
    assert _same_bits(out_only.contiguous(), out.contiguous())
    planes = _run_gather_lm(backend, cfg, table, sset, "x", 1)
    assert _same_bits(planes[:L, :S].contiguous(), out.contiguous())
    h, J = _run_field_gather(backend, cfg, table, sset, "x", 1)
    assert _same_bits(J[:L, :S].contiguous(), jac.contiguous())


# =================================================================================================== b. nsim_lotd_gather_lm
@pytest.mark.parametrize("form", ["x", "rays"])
@pytest.mark.parametrize("S", COUNTS)
def test_gather_lm_point_counts(backend, S, form):
    """both plane types at every block count of the 128-point blocks (and of the with-grad form's 64-point blocks: c), on the
    whole-box set and the 16-level pyramid (five hashed levels split between two XCD groups); the f16 planes are f16(sat(1024 x the f32 planes)) bit for bit; b's f32 planes == c's h_planes"""
    cfg, lv = _lotd("generic", 16)
    sset = _box_set(S)
    table = _table(cfg.n_params)
    ref = gr.lotd_ref(lv, table, sset.points(form))
    L, Z = lv.num_levels, _rows_zeroed(lv.num_levels)
    p32 = _run_gather_lm(backend, cfg, table, sset, form, 1)
    _accept_rows("nsim_lotd_gather_lm", backend, p32, ref.feat, ref.feat_bound(), S, Z)
    p16 = _run_gather_lm(backend, cfg, table, sset, form, 0)
    _accept_f16_feat("nsim_lotd_gather_lm", backend, p16, ref, S, Z)
    assert _same_bits(p16[:Z, :S].contiguous(), _f16_of_f32_planes(p32[:Z, :S]).contiguous())
    for prec in (1, 0):
        h, J = _run_field_gather(backend, cfg, table, sset, form, prec)
        _accept_rows("nsim_field_fwd(gather)", backend, h, ref.feat, ref.feat_bound(), S, Z)
        _accept_J("nsim_field_fwd(gather)", backend, J, ref, S, Z, _jmask(lv, sset, form, sset.name))
        assert _same_bits(h[:Z, :S].contiguous(), p32[:Z, :S].contiguous())


@pytest.mark.parametrize("L", [1, 5, 8, 11, 16, 17, 19, 24, 32])
def test_gather_pyramid_depths(backend, L):
    """1..32 levels: the rows past the pyramid are zeros up to row 16 / the next multiple of 8 and untouched beyond, for the
    no-grad and the with-grad form; levels split between two XCD groups, whole levels, groups with several levels"""
    cfg, lv = _lotd("generic", L)
    Z = _rows_zeroed(L)
    table = _table(cfg.n_params)
    for S in (129, 385):
        sset = _box_set(S)
        ref = gr.lotd_ref(lv, table, sset.points("rays"))
        p32 = _run_gather_lm(backend, cfg, table, sset, "rays", 1)
        _accept_rows("nsim_lotd_gather_lm", backend, p32, ref.feat, ref.feat_bound(), S, Z)
        p16 = _run_gather_lm(backend, cfg, table, sset, "rays", 0)
        _accept_f16_feat("nsim_lotd_gather_lm", backend, p16, ref, S, Z)
        h, J = _run_field_gather(backend, cfg, table, sset, "rays", 0)
        _accept_rows("nsim_field_fwd(gather)", backend, h, ref.feat, ref.feat_bound(), S, Z)
        _accept_J("nsim_field_fwd(gather)", backend, J, ref, S, Z, _jmask(lv, sset, "rays", sset.name))
        assert _same_bits(h[:Z, :S].contiguous(), p32[:Z, :S].contiguous())


# =================================================================================================== c. nsim_field_fwd, gather only
@pytest.mark.parametrize("form", ["x", "rays"])
@pytest.mark.parametrize("name,kind", [("ray200", "generic"), ("interleaved128", "generic"), ("lattice", "lattice"),
                                       ("ray200", "cuboid"), ("box257", "cuboid"), ("ray200", "tiny"), ("box129", "tiny")])
def test_field_gather_sets(backend, name, kind, form):
    """h + dh/dx planes, f32 and f16, on the parity-slot sets (neighbouring lanes in neighbouring cells), ON the cell decisions,
    on a cuboid pyramid over a non-unit AABB and on 16-entry tables; the no-grad enumeration (corner = slot ^ mask) and the
    with-grad one (per-axis operand tables) give the same bits"""
    cfg, lv = _lotd(kind)
    sset = _get_set(name, kind)
    S, Z = sset.S, _rows_zeroed(lv.num_levels)
    table = _table(cfg.n_params)
    ref = gr.lotd_ref(lv, table, sset.points(form))
    mask = _jmask(lv, sset, form, name)
    p32 = _run_gather_lm(backend, cfg, table, sset, form, 1)
    _accept_rows("nsim_lotd_gather_lm", backend, p32, ref.feat, ref.feat_bound(), S, Z)
    for prec in (1, 0):
        h, J = _run_field_gather(backend, cfg, table, sset, form, prec)
        _accept_rows("nsim_field_fwd(gather)", backend, h, ref.feat, ref.feat_bound(), S, Z)
        _accept_J("nsim_field_fwd(gather)", backend, J, ref, S, Z, mask)
        assert _same_bits(h[:Z, :S].contiguous(), p32[:Z, :S].contiguous())


# =================================================================================================== n_dev / n_add
@pytest.mark.parametrize("n_valid", [0, 1, 64, 65, 128, 129, 385, 386])
def test_gather_device_side_count(backend, n_valid):
    """capacity 385, the valid count n_dev[0] + n_add read on the device: (level, point < count) exactly once, nothing at or past
    the count (the split of a level is by halves of the VALID range); a count above the capacity touches nothing"""
    cfg, lv = _lotd("generic", 16)
    sset = _box_set(385)
    table = _table(cfg.n_params)
    ref = gr.lotd_ref(lv, table, sset.points("x"))
    Sv = n_valid if n_valid <= 385 else 0
    Z = _rows_zeroed(lv.num_levels) if Sv else 0
    p32 = _run_gather_lm(backend, cfg, table, sset, "x", 1, n_valid=n_valid)
    _accept_rows("nsim_lotd_gather_lm", backend, p32, ref.feat, ref.feat_bound(), Sv, Z)
    p16 = _run_gather_lm(backend, cfg, table, sset, "x", 0, n_valid=n_valid, n_add=0)
    _accept_f16_feat("nsim_lotd_gather_lm", backend, p16, ref, Sv, Z)
    h, J = _run_field_gather(backend, cfg, table, sset, "x", 0, n_valid=n_valid)
    _accept_rows("nsim_field_fwd(gather)", backend, h, ref.feat, ref.feat_bound(), Sv, Z)
    _accept_J("nsim_field_fwd(gather)", backend, J, ref, Sv, Z, _jmask(lv, sset, "x", sset.name))
    pc, pm = _permuto(3)
    tp = _table(pc.n_params)
    rp = gr.permuto_ref(pm, tp, sset.points("x"))
    f32p, hp, Jp = _run_permuto(backend, pc, tp, sset, "x", None, "f32", n_valid=n_valid)
    _accept_rows("nsim_permuto_gather", backend, f32p, rp.feat, rp.feat_bound(), Sv, 16 if Sv else 0)
    _accept_rows("nsim_permuto_gather", backend, hp, rp.feat, rp.feat_bound(), Sv, 16 if Sv else 0)
    _accept_J("nsim_permuto_gather", backend, Jp, rp, Sv, 16 if Sv else 0, torch.zeros(pm.num_levels, 385, dtype=torch.bool))


# =================================================================================================== n_active_levels
@pytest.mark.parametrize("L,n_active", [(10, 1), (10, 4), (10, 9), (19, 12)])
def test_masked_levels(backend, L, n_active):
    """hardmask: masked rows are zeros; their table region is NaN in the table the kernels get (a read would surface); the
    active levels' outputs are the unmasked run's, bit for bit"""
    cfg, lv = _fresh_lotd("generic", L)
    sset = _box_set(257)
    S, Z = sset.S, _rows_zeroed(L)
    table = _table(cfg.n_params)
    full32 = _run_gather_lm(backend, cfg, table, sset, "rays", 1)
    full_h, full_J = _run_field_gather(backend, cfg, table, sset, "rays", 0)
    full_out, full_jac = _run_lotd_fwd(backend, cfg, table, sset)
    cfg.set_active_levels(n_active)
    masked = table.clone()
    masked[lv.offsets[n_active]:] = float("nan")
    ref = gr.lotd_ref(lv, table, sset.points("rays"), n_active=n_active)
    assert not bool(ref.feat[n_active:].any()) and not bool(ref.feat_bound()[n_active:].any())
    mask = _jmask(lv, sset, "rays", sset.name)
    p32 = _run_gather_lm(backend, cfg, masked, sset, "rays", 1)
    _accept_rows("nsim_lotd_gather_lm", backend, p32, ref.feat, ref.feat_bound(), S, Z)
    assert _same_bits(p32[:n_active, :S].contiguous(), full32[:n_active, :S].contiguous())
    p16 = _run_gather_lm(backend, cfg, masked, sset, "rays", 0)
    _accept_f16_feat("nsim_lotd_gather_lm", backend, p16, ref, S, Z)
    h, J = _run_field_gather(backend, cfg, masked, sset, "rays", 0)
    _accept_rows("nsim_field_fwd(gather)", backend, h, ref.feat, ref.feat_bound(), S, Z)
    _accept_J("nsim_field_fwd(gather)", backend, J, ref, S, Z, mask)
    assert _same_bits(h[:n_active, :S].contiguous(), full_h[:n_active, :S].contiguous())
    assert _same_bits(J[:n_active, :S].contiguous(), full_J[:n_active, :S].contiguous())
    refx = gr.lotd_ref(lv, table, sset.points("x"), n_active=n_active)
    out, jac = _run_lotd_fwd(backend, cfg, masked, sset)
    _accept_rows("nsim_lotd_fwd", backend, out, refx.feat, refx.feat_bound(), S, L)
    _accept_rows("nsim_lotd_fwd", backend, jac, refx.J, refx.J_bound(), S, L, _jmask(lv, sset, "x", sset.name))
    assert _same_bits(out[:n_active].contiguous(), full_out[:n_active].contiguous())
    assert _same_bits(jac[:n_active].contiguous(), full_jac[:n_active].contiguous())
    # the hess term sums the active levels only (g of the masked levels is NaN: never read)
    gen = torch.Generator().manual_seed(5)
    g, gn, dx0 = torch.randn(L, S, 2, generator=gen), torch.randn(S, 3, generator=gen), torch.randn(S, 3, generator=gen)
    g_dev = g.clone()
    g_dev[n_active:] = float("nan")
    g[n_active:] = 0.0
    val, bnd = gr.hess_dx(refx, g.double(), gn.double(), dx0.double())
    dx = _run_hess(backend, cfg, masked, sset, "x", g_dev, gn, dx0)
    keep = (_pair_margin(lv, sset.points("x"))[:n_active] >= sr.MARGIN).all(0)
    assert bool(torch.isfinite(dx).all())
    worst = gr.ratio((dx.double() - val).abs()[keep], bnd[keep])
    print(f"RATIO nsim_lotd_hess_dx {_dev_name(backend)} {worst:.4f}")
    assert worst <= 1.0


# =================================================================================================== ray_goff
@pytest.mark.parametrize("form", ["x", "rays"])
def test_batched_instances(backend, form):
    """two instances in one flat table (even offsets), the offset read through ridx: b, c and d.  Neighbouring lanes sit in the
    same cell of different instances"""
    cfg, lv = _lotd()
    sset = _margin_set("batched")
    S, L, Z = sset.S, lv.num_levels, _rows_zeroed(lv.num_levels)
    table = _table(2 * cfg.n_params + 64)
    goff = torch.tensor([64, cfg.n_params + 64], dtype=torch.long)
    ref = gr.lotd_ref(lv, table, sset.points(form), goff=goff[sset.ridx])
    alone = gr.lotd_ref(lv, table[64:64 + cfg.n_params], sset.points(form))
    assert torch.equal(ref.feat[:, 0::2], alone.feat[:, 0::2]) and not torch.equal(ref.feat[:, 1::2], alone.feat[:, 1::2])
    mask = _jmask(lv, sset, form, "batched")
    p32 = _run_gather_lm(backend, cfg, table, sset, form, 1, goff=goff)
    _accept_rows("nsim_lotd_gather_lm", backend, p32, ref.feat, ref.feat_bound(), S, Z)
    p16 = _run_gather_lm(backend, cfg, table, sset, form, 0, goff=goff)
    _accept_f16_feat("nsim_lotd_gather_lm", backend, p16, ref, S, Z)
    for prec in (1, 0):
        h, J = _run_field_gather(backend, cfg, table, sset, form, prec, goff=goff)
        _accept_rows("nsim_field_fwd(gather)", backend, h, ref.feat, ref.feat_bound(), S, Z)
        _accept_J("nsim_field_fwd(gather)", backend, J, ref, S, Z, mask)
    gen = torch.Generator().manual_seed(6)
    g, gn, dx0 = torch.randn(L, S, 2, generator=gen), torch.randn(S, 3, generator=gen), torch.randn(S, 3, generator=gen)
    val, bnd = gr.hess_dx(ref, g.double(), gn.double(), dx0.double())
    dx = _run_hess(backend, cfg, table, sset, form, g, gn, dx0, goff=goff)
    worst = gr.ratio((dx.double() - val).abs(), bnd)
    print(f"RATIO nsim_lotd_hess_dx {_dev_name(backend)} {worst:.4f}")
    assert worst <= 1.0


# =================================================================================================== d. nsim_lotd_hess_dx
@pytest.mark.parametrize("form", ["x", "rays"])
@pytest.mark.parametrize("name,kind", [("ray200", "generic"), ("interleaved128", "generic"), ("ray65", "generic"),
                                       ("lattice", "lattice"), ("ray200", "cuboid"), ("ray200", "tiny")])
def test_hess_dx(backend, name, kind, form):
    """the mixed second derivatives contracted with g and gn, ADDED to a pre-filled dx; g_planes at pitch S (S = 200, 65, 66:
    no multiple of 32 -- a plane pitch in its place reads another point's g)"""
    cfg, lv = _lotd(kind)
    sset = _get_set(name, kind)
    S, L = sset.S, lv.num_levels
    assert _jmask(lv, sset, form, name).all()
    table = _table(cfg.n_params)
    ref = gr.lotd_ref(lv, table, sset.points(form))
    gen = torch.Generator().manual_seed(7)
    g, gn, dx0 = torch.randn(L, S, 2, generator=gen), torch.randn(S, 3, generator=gen), 100.0 * torch.randn(S, 3, generator=gen)
    val, bnd = gr.hess_dx(ref, g.double(), gn.double(), dx0.double())
    dx = _run_hess(backend, cfg, table, sset, form, g, gn, dx0)
    assert bool(torch.isfinite(dx).all())
    worst = gr.ratio((dx.double() - val).abs(), bnd)
    print(f"RATIO nsim_lotd_hess_dx {_dev_name(backend)} {worst:.4f}")
    assert worst <= 1.0
    if name != "lattice":                                                               # the term itself is far above the bound
        assert float(((val - dx0.double()).abs() > 8 * bnd).double().mean()) > 0.5


# =================================================================================================== saturation
def test_f16_planes_saturate(backend):
    """features beyond 63.97 (x 1024 > 65504) and dh/dx beyond 65504 on the fine levels: the f16 planes hold +-65504, never inf"""
    cfg, lv = _lotd("generic", 16)
    sset = _margin_set("ray200")
    S, Z = sset.S, 16
    table = _table(cfg.n_params, seed=9, amp=400.0)
    ref = gr.lotd_ref(lv, table, sset.points("x"))
    assert float(ref.feat.abs().max()) > 63.97 and float(ref.J[10:].abs().max()) > gr.F16_MAX
    mask = _pair_margin(lv, sset.points("x")) >= sr.MARGIN
    p16 = _run_gather_lm(backend, cfg, table, sset, "x", 0)
    _accept_f16_feat("nsim_lotd_gather_lm", backend, p16, ref, S, Z)
    big = ref.feat.abs() > 64.0 + ref.feat_bound()
    assert bool(big.any()) and bool((p16[:16, :S].double().abs()[big] == gr.F16_MAX).all())
    h, J = _run_field_gather(backend, cfg, table, sset, "x", 0)
    _accept_rows("nsim_field_fwd(gather)", backend, h, ref.feat, ref.feat_bound(), S, Z)
    _accept_J("nsim_field_fwd(gather)", backend, J, ref, S, Z, mask)
    bigJ = (ref.J.abs() > 1.01 * gr.F16_MAX + ref.J_bound()) & mask[:, :, None, None]
    assert bool(bigJ.any()) and bool((J[:16, :S].double().abs()[bigJ] == gr.F16_MAX).all())
    pc, pm = _permuto(3)
    tp = _table(pc.n_params, seed=9, amp=30000.0)
    ps = _permuto_set("ray200", 3)
    rp = gr.permuto_ref(pm, tp, ps.points("x"))
    assert float(rp.J.abs().max()) > gr.F16_MAX
    f16p, hp, Jp = _run_permuto(backend, pc, tp, ps, "x", None, "f16")
    _accept_f16_feat("nsim_permuto_gather", backend, f16p, rp, ps.S, 16)
    _accept_J("nsim_permuto_gather", backend, Jp, rp, ps.S, 16, torch.ones(pm.num_levels, ps.S, dtype=torch.bool))
    assert bool((Jp[:pm.num_levels, :ps.S].double().abs()[rp.J.abs() > 1.01 * gr.F16_MAX + rp.J_bound()] == gr.F16_MAX).all())


# =================================================================================================== e. nsim_permuto_gather
@functools.lru_cache(maxsize=None)
def _permuto(D, log2_T=10, L=6):
    pc = PermutoConfig(in_dim=D, n_levels=L, n_feats=2, log2_hashmap_size=log2_T, coarsest_res=1.5, finest_res=160.0, seed=3)
    return pc, sr.permuto_levels(pc)


def _z(D, n_rays):
    g = torch.Generator().manual_seed(40 + D)
    return torch.rand(n_rays, D - 3, generator=g) * 2 - 1


@functools.lru_cache(maxsize=None)
def _permuto_set(name, D, L=6):
    """3-D sets whose rays carry the condition of a D-dimensional lattice; the margin-keeping ones are settled on the lattice"""
    if name.startswith("box"):
        return _box_set(int(name[3:]))
    pm = _permuto(D, 10, L)[1]
    n_rays = 2 if name.startswith("interleaved") else 1
    kw = dict(margin_fn=sr.permuto_margin(pm, None if D == 3 else _z(D, n_rays)))
    if name.startswith("interleaved"):
        return sr.interleaved(int(name[11:]), **kw)
    return sr.dense_ray(int(name[3:]), **kw)


def _permuto_points(sset, form, D):
    p = sset.points(form)
    return p if D == 3 else torch.cat([p, _z(D, int(sset.o.shape[0])).double()[sset.ridx]], dim=1)


def _run_permuto(device, pc, table, sset, form, z, mode, n_valid=None, n_add=2):
    """mode "f16" / "f32" -> (feat_planes of a no-grad call, h_planes, J_planes of a with-grad call)"""
    S, L = sset.S, pc.num_levels
    f32 = mode == "f32"
    P = _lib.plane_pitch(S)
    feat = torch.empty(_nlp(L), P, 2, dtype=torch.float32 if f32 else torch.float16, device=device)
    h = torch.empty(_nlp(L), P, 2, dtype=torch.float32, device=device)
    J = torch.empty(_nlp(L), P, 2, 3, dtype=torch.float32 if f32 else torch.float16, device=device)
    x, o, d, t, ridx = _pt_args(sset, form, device, z is not None)
    tab, zd, nd = _dv(table, device), _dv(z, device), _n_dev(n_valid, n_add, device)
    na = n_add if n_valid is not None else 0
    _lib.call("nsim_permuto_gather", pc.meta, _lib.ptr(tab), _lib.ptr(x), _lib.ptr(o), _lib.ptr(d), _lib.ptr(t), _lib.ptr(ridx),
              _lib.ptr(zd), S, _lib.ptr(nd), na, _lib.ptr(feat), int(f32), None, None)
    _lib.call("nsim_permuto_gather", pc.meta, _lib.ptr(tab), _lib.ptr(x), _lib.ptr(o), _lib.ptr(d), _lib.ptr(t), _lib.ptr(ridx),
              _lib.ptr(zd), S, _lib.ptr(nd), na, None, int(f32), _lib.ptr(h), _lib.ptr(J))
    _sync(device)
    return feat.cpu(), h.cpu(), J.cpu()


@pytest.mark.parametrize("form", ["x", "rays"])
@pytest.mark.parametrize("name", ["ray200", "interleaved128", "ray65", "box257", "box1"])
@pytest.mark.parametrize("D", [3, 5])
def test_permuto_gather(backend, D, name, form):
    """feature planes f16 and f32, h + dh/dx planes f16 and f32, with (in_dim 5) and without a per-ray condition; rows 6..15 are
    zeros (the 16-level decoders read them), rows >= 16 do not exist; f32 feature planes == h_planes bit for bit.  dh/dx is
    constant inside a simplex: compared on the margin-keeping sets (permuto_margin, asserted)"""
    pc, pm = _permuto(D)
    sset = _permuto_set(name, D)
    S, L = sset.S, pm.num_levels
    z = None if D == 3 else _z(D, int(sset.o.shape[0]))
    table = _table(pc.n_params)
    ref = gr.permuto_ref(pm, table, _permuto_points(sset, form, D))
    with_J = not name.startswith("box")
    if with_J:
        fn = sr.permuto_margin(pm, z)
        m = min(fn(sset, "rays"), fn(sset, "x"))
        assert m >= sr.MARGIN, f"{sset.name}: decision margin {m}"
    mask = torch.full((L, S), with_J, dtype=torch.bool)
    f32p, h32, J32 = _run_permuto(backend, pc, table, sset, form, z, "f32")
    f16p, h16, J16 = _run_permuto(backend, pc, table, sset, form, z, "f16")
    _accept_rows("nsim_permuto_gather", backend, f32p, ref.feat, ref.feat_bound(), S, 16)
    _accept_f16_feat("nsim_permuto_gather", backend, f16p, ref, S, 16)
    assert _same_bits(f16p[:16, :S].contiguous(), _f16_of_f32_planes(f32p[:16, :S]).contiguous())
    for h, J in ((h32, J32), (h16, J16)):
        _accept_rows("nsim_permuto_gather", backend, h, ref.feat, ref.feat_bound(), S, 16)
        _accept_J("nsim_permuto_gather", backend, J, ref, S, 16, mask)
        assert _same_bits(h[:16, :S].contiguous(), f32p[:16, :S].contiguous())
    assert _same_bits(J16[:16, :S].contiguous(), J32[:16, :S].clamp(-gr.F16_MAX, gr.F16_MAX).half().contiguous())


@pytest.mark.parametrize("L,n_active", [(6, 0), (16, 0), (19, 0), (19, 7), (6, 2)])
def test_permuto_gather_rows_and_masked_levels(backend, L, n_active):
    """rows past the pyramid: zeros up to 16 / the next multiple of 8, untouched beyond; masked levels: zeros, their table NaN,
    the active levels bit-identical to the unmasked run"""
    pc = PermutoConfig(in_dim=3, n_levels=L, n_feats=2, log2_hashmap_size=9, coarsest_res=1.5, finest_res=160.0, seed=3)
    pm = sr.permuto_levels(pc)
    sset = _box_set(257)
    S, Z = sset.S, _rows_zeroed(L)
    table = _table(pc.n_params)
    full, full_h, _ = _run_permuto(backend, pc, table, sset, "rays", None, "f32")
    ref = gr.permuto_ref(pm, table, sset.points("rays"), n_active=n_active or None)
    if n_active:
        pc.meta.n_active_levels = n_active
        table = table.clone()
        table[n_active * pm.T * 2:] = float("nan")
    for mode in ("f32", "f16"):
        fp, h, J = _run_permuto(backend, pc, table, sset, "rays", None, mode)
        if mode == "f32":
            _accept_rows("nsim_permuto_gather", backend, fp, ref.feat, ref.feat_bound(), S, Z)
            assert _same_bits(fp[:n_active or L, :S].contiguous(), full[:n_active or L, :S].contiguous())
        else:
            _accept_f16_feat("nsim_permuto_gather", backend, fp, ref, S, Z)
        _accept_rows("nsim_permuto_gather", backend, h, ref.feat, ref.feat_bound(), S, Z)
        _accept_J("nsim_permuto_gather", backend, J, ref, S, Z, torch.zeros(L, S, dtype=torch.bool))
        assert _same_bits(h[:n_active or L, :S].contiguous(), full_h[:n_active or L, :S].contiguous())
        assert not bool(J[n_active or L:Z, :S].double().abs().any())


# =================================================================================================== f. the 4-D gather
@functools.lru_cache(maxsize=None)
def _lotd4(L=6):
    res_xyz, res_w, T = [3, 4, 6, 9, 17, 40, 60, 90, 130, 200, 300, 512][:L], [2, 3, 4, 7, 12, 30, 40, 50, 64, 80, 100, 128][:L], 2 ** 9
    types, sizes, offs, off = [], [], [], 0
    for rx, rw in zip(res_xyz, res_w):
        n = rx ** 3 * rw
        types.append("Dense" if n <= T else "Hash")
        sizes.append(n if n <= T else T)
        offs.append(off)
        off += sizes[-1] * 2
    spec = odist.LoTD4Spec(res_xyz, res_w, types, sizes, offs, off, T)
    m = _lib.DistantMeta()
    m.lotd.num_levels = spec.num_levels
    for l in range(spec.num_levels):
        m.lotd.res_xyz[l], m.lotd.res_w[l], m.lotd.type[l] = res_xyz[l], res_w[l], 0 if types[l] == "Dense" else 1
        m.lotd.size[l], m.lotd.offset[l] = sizes[l], offs[l]
    m.precision = 1
    return spec, m


def _run_distant_gather(device, spec, meta, table, u4):
    """nsim_distant_fwd(..., h_planes) with finite decoder weights -> h_planes [16, S, 2]"""
    S, F = int(u4.shape[0]), 2 * spec.num_levels
    g = torch.Generator().manual_seed(2)
    den_w, den_b = 0.1 * torch.randn(64 * F + 64, generator=g), torch.zeros(65)
    rad_w, rad_b = 0.1 * torch.randn(64 * (F + 20) + 4096 + 192, generator=g), torch.zeros(131)
    wpack = torch.zeros(int(_lib.get_lib().nsim_distant_wpack_bytes(meta)), dtype=torch.uint8, device=device)
    _lib.call("nsim_distant_pack_weights", meta, _lib.ptr(_dv(den_w, device)), _lib.ptr(_dv(den_b, device)),
              _lib.ptr(_dv(rad_w, device)), _lib.ptr(_dv(rad_b, device)), _lib.ptr(wpack))
    rays_d = _dv(sr._unit(sr._DIR[:3]).float().expand(S, 3), device)
    sigma, rgb = torch.empty(S, dtype=torch.float32, device=device), torch.empty(S, 3, dtype=torch.float32, device=device)
    h = torch.empty(16, S, 2, dtype=torch.float32, device=device)
    _lib.call("nsim_distant_fwd", meta, _lib.ptr(_dv(table, device)), _lib.ptr(wpack), _lib.ptr(_dv(u4, device)), _lib.ptr(rays_d),
              None, S, 1, _lib.ptr(sigma), _lib.ptr(rgb), _lib.ptr(h))
    _sync(device)
    return h.cpu()


@pytest.mark.parametrize("S", COUNTS)
def test_distant_gather_point_counts(backend, S):
    """the 4-D level-major gather: u over [-0.2, 1.2]^4 with u = 0, 1 (top face: last cell, w = 1), the mid planes and points
    beyond the box (clamped cell, extrapolating weights -- ``lotd4_cell``); levels split by halves of the launch's blocks.
    The pyramid's rows at pitch S; rows num_levels .. 15 are NOT written (the distant decoders guard every row)"""
    spec, meta = _lotd4()
    sset = gr.whole_box(S, dim=4, box=(0.0, 1.0))
    u4 = sset.x32()
    if S >= 63:
        assert bool((u4 == 0).any()) and bool((u4 == 1).any()) and bool((u4 > 1).any()) and bool((u4 < 0).any())
    table = _table(spec.n_params)
    ref = gr.lotd4_ref(spec, table, u4.double())
    h = _run_distant_gather(backend, spec, meta, table, u4)
    _accept_rows("nsim_distant_fwd(gather)", backend, h, ref.feat, ref.feat_bound(), S, spec.num_levels)


@pytest.mark.parametrize("L", [1, 3, 12])
def test_distant_gather_depths(backend, L):
    """1 and 3 levels (XCD groups without a level) and 12: ten hashed levels, two of them split by halves of the blocks"""
    spec, meta = _lotd4(L)
    for S in (129, 385):
        u4 = gr.whole_box(S, dim=4, box=(0.0, 1.0)).x32()
        table = _table(spec.n_params)
        ref = gr.lotd4_ref(spec, table, u4.double())
        h = _run_distant_gather(backend, spec, meta, table, u4)
        _accept_rows("nsim_distant_fwd(gather)", backend, h, ref.feat, ref.feat_bound(), S, L)


# =================================================================================================== random compositions
@settings(**SET)
@given(L=st.integers(1, 32), S=st.integers(1, 400), frac=st.sampled_from([None, 0.0, 0.3, 0.5, 0.51, 1.0, 1.01]),
       form=st.sampled_from(["x", "rays"]), prec=st.integers(0, 1), seed=st.integers(0, 10 ** 6))
def test_gather_random_compositions(backend, L, S, frac, form, prec, seed):
    """exactly-once / nothing-else and the bound on random (num_levels, capacity, valid count, form)"""
    cfg, lv = _lotd("generic", L)
    sset = gr.whole_box(S, seed=seed)
    n_valid = None if frac is None else min(S + 1, int(round(frac * S)) + (1 if frac > 1 else 0))
    Sv = S if n_valid is None else (n_valid if n_valid <= S else 0)
    Z = _rows_zeroed(L) if Sv else 0
    table = _table(cfg.n_params, seed=seed)
    ref = gr.lotd_ref(lv, table, sset.points(form))
    pl = _run_gather_lm(backend, cfg, table, sset, form, prec, n_valid=n_valid)
    if prec:
        _accept_rows("nsim_lotd_gather_lm", backend, pl, ref.feat, ref.feat_bound(), Sv, Z)
    else:
        _accept_f16_feat("nsim_lotd_gather_lm", backend, pl, ref, Sv, Z)
    h, J = _run_field_gather(backend, cfg, table, sset, form, prec, n_valid=n_valid)
    _accept_rows("nsim_field_fwd(gather)", backend, h, ref.feat, ref.feat_bound(), Sv, Z)
    _accept_J("nsim_field_fwd(gather)", backend, J, ref, Sv, Z, _pair_margin(lv, sset.points(form)) >= sr.MARGIN)
