"""The table-gradient scatters on coherent, run-heavy sample sets, entry point by entry point, against float64 contribution
lists (tests/scatter_ref.py): ``nsim_lotd_scatter``, ``nsim_lotd4_scatter``, ``nsim_permuto_bwd``, ``nsim_permuto_scatter``,
``nsim_permuto_scatter_pts``, ``nsim_permuto_dz`` -- the four kernels that share the wave-level run merge (ballot of run heads,
segmented shuffle scan, the run's last lane emits; parity slots and quad-transposed atomics in the two LoTD ones) --, with
``nsim_lotd_bwd`` (no merge) as the control and ``nsim_ray_grad_reduce`` (atomics on a handful of addresses per wave).
The planes are built here: no decoder is involved.

Sets (scatter_ref.py): identical points (S = 1, 63, 64, 65, 130, 257), staggered run lengths, a dense ray (64 / 200 samples),
two rays interleaved lane by lane, holes in ``valid``, lattice points, a 16-entry hash table, two batched instances alternating
inside one cell, and random compositions of runs (hypothesis).  The generic sets keep a decision margin of 1e-3 (asserted).

Bound, per table entry e (derived, not measured -- scatter_ref.bound):  |got_e - ref_e| <= (n_e + r_l + 16) 2^-24 A_e,
r_l = 3 R_l (4 R_l in 4-D, (in_dim + 1) x the level's largest scale on the lattice); untouched entries and masked levels are
exactly 0.0.  ``nsim_permuto_dz`` and ``nsim_ray_grad_reduce`` sum products of inputs and simplex constants, nothing with an
absolute weight error: (n_e + 16) 2^-24 sum |term| (scatter_ref.per_term_bound).

Worst observed error / bound over all cases of this file (every case prints its own as ``RATIO <entry point> <device> <value>``):

    entry point                 emulator    MI355X
    nsim_lotd_scatter           0.1145      0.1145
    nsim_lotd4_scatter          0.0448      0.0448
    nsim_permuto_bwd            0.0374      0.0374
    nsim_permuto_scatter        0.0145      0.0145
    nsim_permuto_scatter_pts    0.0028      0.0028
    nsim_permuto_dz             0.0005      0.0004
    nsim_lotd_bwd               0.0486      0.0486
    nsim_ray_grad_reduce        0.0235      0.0277

(The library is compiled with -ffp-contract=off, as the emulator: the weights are the same bits on both, what differs is the
order of the atomic sums.  The decision margin is what the comparison with float64 needs either way.)
"""
import functools
import os

import pytest
import torch
from hypothesis import HealthCheck, given, settings, strategies as st

import scatter_ref as sr
from oracle import distant as odist, lotd as olotd, permuto as operm
from neuralsim_amd import _lib
from neuralsim_amd.grid_encodings.lotd import LoTDConfig
from neuralsim_amd.grid_encodings.permuto import PermutoConfig

# NSIM_FUZZ_EXAMPLES=N: an exploratory sweep with fresh random examples (the convention of the fuzz files); derandomized by default
_N = int(os.environ.get("NSIM_FUZZ_EXAMPLES", "0"))
SET = dict(max_examples=_N or 12, derandomize=_N == 0, deadline=None,
           suppress_health_check=[HealthCheck.function_scoped_fixture])

LOTD_RES = [3, 5, 8, 9, 11, 17, 33, 67, 129, 257]        # T = 2^9: 3, 5, 8 dense, 9 and finer hashed
F64 = torch.float64


def _sync(device):
    if device.type == "cuda":
        torch.cuda.synchronize()


def _dv(t, device):
    return None if t is None else t.to(device).contiguous()


def _accept(got, contribs, name, device, per_term=False):
    ok, worst = sr.check(got, contribs, per_term)
    print(f"RATIO {name} {'hip' if device.type == 'cuda' else 'emu'} {worst:.4f}")
    assert ok, f"{name}: worst error / bound = {worst} (or an untouched entry is not 0.0)"
    return worst


def _upstream(L, S, seed, nq=3):
    """dh, g [L,S,2], gn [S,nq]: unscaled randn (so that one sample more or less is far above the bound)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(L, S, 2, generator=g), torch.randn(L, S, 2, generator=g), torch.randn(S, nq, generator=g)


def _q(g, gn):
    return g.double()[:, :, :, None] * gn.double()[None, :, None, :]


# ------------------------------------------------------------------------------------------------- pyramids and sets
@functools.lru_cache(maxsize=None)
def _lotd(kind="generic"):
    if kind == "generic":
        cfg = LoTDConfig(LOTD_RES, 2, 9)
    elif kind == "lattice":
        cfg = LoTDConfig(sr.LATTICE_RES, 2, 8)
    elif kind == "tiny":
        cfg = LoTDConfig([2, 3, 5, 9, 17, 33], 2, 4)
    elif kind == "cuboid":
        cfg = LoTDConfig([[3, 4, 5], [5, 7, 9], [9, 13, 17], [17, 25, 33], [40, 60, 80]], 2, 9)
        cfg.set_aabb([[-1.0, -1.5, -2.0], [1.0, 1.5, 2.0]])
    return cfg, sr.lotd_levels(cfg)


def _fresh_lotd(kind="generic"):
    """a config of its own for the tests that change the meta (n_active_levels)"""
    return _lotd.__wrapped__(kind)


@functools.lru_cache(maxsize=None)
def _lotd_set(name, kind="generic"):
    lv = _lotd(kind)[1]
    kw = dict(margin_fn=sr.lotd_margin(lv))
    if kind == "cuboid":
        kw["box"] = ([-1.0, -1.5, -2.0], [1.0, 1.5, 2.0])
    if name.startswith("identical"):
        return sr.identical(int(name[9:]), **kw)
    if name == "staggered":
        return sr.staggered(**kw)
    if name.startswith("ray"):
        return sr.dense_ray(int(name[3:]), **kw)
    if name.startswith("interleaved"):
        return sr.interleaved(int(name[11:]), **kw)
    if name == "batched":
        return sr.batched_pair(200, **kw)
    raise KeyError(name)


LOTD_SETS = [f"identical{S}" for S in sr.IDENTICAL_S] + ["staggered", "ray64", "ray200", "interleaved128"]


def _lotd_scatter(device, cfg, sset, form, dh, g, gn, goff=None, n_entries=None, begin=0, count=0, dgrid=None):
    if dgrid is None:
        dgrid = torch.zeros(n_entries or cfg.n_params, dtype=torch.float32, device=device)
    if form == "x":
        x, o, d, t = _dv(sset.x32(), device), None, None, None
        ridx = _dv(sset.ridx, device) if goff is not None else None
    else:
        x, o, d, t, ridx = None, _dv(sset.o, device), _dv(sset.d, device), _dv(sset.t, device), _dv(sset.ridx, device)
    _lib.call("nsim_lotd_scatter", cfg.meta, _lib.ptr(x), _lib.ptr(o), _lib.ptr(d), _lib.ptr(t), _lib.ptr(ridx),
              _lib.ptr(_dv(goff, device)), sset.S, _lib.ptr(_dv(dh, device)), _lib.ptr(_dv(g, device)), _lib.ptr(_dv(gn, device)),
              _lib.ptr(dgrid), begin, count)
    _sync(device)
    return dgrid


def _margin_ok(fn, sset):
    m = min(fn(sset, "rays"), fn(sset, "x"))
    assert m >= sr.MARGIN, f"{sset.name}: decision margin {m}"


# =================================================================================================== the comparison bites
@pytest.mark.parametrize("name", ["staggered", "ray200"])
def test_comparison_rejects_a_dropped_and_a_doubled_sample(name):
    """CPU only: the reference list of sets 2 and 3 with its smallest-magnitude sample removed, and with one sample added
    twice, must both be rejected (and the untouched list accepted)"""
    cfg, lv = _lotd()
    sset = _lotd_set(name)
    dh, g, gn = _upstream(lv.num_levels, sset.S, 5)
    c = sr.lotd_contribs(lv, sset.points("x"), dh.double(), _q(g, gn))
    assert sr.check(c.gradient().float(), c)[0]
    mag = torch.zeros(sset.S, dtype=F64).index_add_(0, c.sample, c.value.abs())
    smallest = int(mag.argmin())
    dropped = c.select(c.sample != smallest).gradient().float()
    ok, worst = sr.check(dropped, c)
    print("dropped sample", smallest, "worst error / bound", worst)
    assert not ok and worst > 1.0
    twice = (c.gradient() + c.select(c.sample == smallest).gradient()).float()
    ok, worst = sr.check(twice, c)
    print("doubled sample", smallest, "worst error / bound", worst)
    assert not ok and worst > 1.0


def test_comparison_rejects_a_stray_write_and_nan():
    cfg, lv = _lotd()
    sset = _lotd_set("identical65")
    dh, g, gn = _upstream(lv.num_levels, sset.S, 5)
    c = sr.lotd_contribs(lv, sset.points("x"), dh.double(), None)
    got = c.gradient().float()
    untouched = int((torch.zeros(c.n_entries).index_add_(0, c.entry, torch.ones(c.entry.shape[0])) == 0).nonzero()[0])
    stray = got.clone()
    stray[untouched] = 1e-30
    assert not sr.check(stray, c)[0]
    stray[untouched] = float("nan")
    assert not sr.check(stray, c)[0]


# =================================================================================================== lists == oracle autograd
def test_reference_lists_equal_oracle_autograd():
    """the contribution lists' ``index_add`` is autograd through oracle/lotd.py (second-order term in the ``create_graph`` form
    of test_field.py::test_lotd_fwd_dydx_bwd), oracle/distant.py::lotd4_forward and oracle/permuto.py on a f64 table leaf"""
    cfg, lv = _lotd()
    sset = _lotd_set("ray64")
    S, L = sset.S, lv.num_levels
    dh, g, gn = _upstream(L, S, 6)
    spec = olotd.make_lotd_spec(LOTD_RES, 2, 9)
    x = sset.points("x").clone().requires_grad_(True)
    table = torch.zeros(spec.n_params, dtype=F64, requires_grad=True)
    h = olotd.lotd_forward(x, table, spec)                                       # [S, 2 L]
    sdf = (h * g.double().permute(1, 0, 2).reshape(S, 2 * L)).sum()               # d sdf / d h = g
    nablas, = torch.autograd.grad(sdf, x, create_graph=True)
    ((h * dh.double().permute(1, 0, 2).reshape(S, 2 * L)).sum() + (nablas * gn.double()).sum()).backward()
    ref = sr.lotd_contribs(lv, sset.points("x"), dh.double(), _q(g, gn)).gradient()
    assert (ref - table.grad).abs().max() <= 1e-12 * table.grad.abs().max()
    # 4-D (the oracle gathers in f32: agreement to its rounding)
    spec4 = _lotd4()[0]
    s4 = _lotd4_set("ray64")
    u = s4.points("x")
    t4 = torch.zeros(spec4.n_params, requires_grad=True)
    dh4 = _upstream(spec4.num_levels, s4.S, 7)[0]
    (odist.lotd4_forward(u.float(), t4, spec4) * dh4.permute(1, 0, 2).reshape(s4.S, -1)).sum().backward()
    ref4 = sr.lotd4_contribs(spec4, u, dh4.double()).gradient()
    assert (ref4 - t4.grad.double()).abs().max() <= 1e-5 * t4.grad.abs().max()
    # permutohedral, with the second-order term
    for D in (3, 5):
        pc, pm = _permuto(D)
        sp = _permuto_set("ray64", D)
        p = sp.points("x") if D == 3 else torch.cat([sp.points("x"), _z(D, sp)[sp.ridx].double()], dim=1)
        Lp = pm.num_levels
        dhp, gp, gnp = _upstream(Lp, sp.S, 8)
        ospec = operm.PermutoSpec(D, list(pc.res), 2, pm.T, pm.shift.float())
        ospec.scale_factors = lambda l, pm=pm: pm.scale[l]                       # the meta's f32 values
        xp = p.clone().requires_grad_(True)
        tp = torch.zeros(pm.n_params, dtype=F64, requires_grad=True)
        hp = operm.permuto_forward(xp, tp, ospec)
        nab, = torch.autograd.grad((hp * gp.double().permute(1, 0, 2).reshape(sp.S, -1)).sum(), xp, create_graph=True)
        ((hp * dhp.double().permute(1, 0, 2).reshape(sp.S, -1)).sum() + (nab[:, :3] * gnp.double()).sum()).backward()
        refp = sr.permuto_contribs(pm, p, dhp.double(), gp.double(), gnp.double()).gradient()
        assert (refp - tp.grad).abs().max() <= 1e-11 * tp.grad.abs().max()


# =================================================================================================== nsim_lotd_scatter
@pytest.mark.parametrize("form", ["x", "rays"])
@pytest.mark.parametrize("name", LOTD_SETS)
def test_lotd_scatter_sets(backend, monkeypatch, name, form):
    """sets 1-4 in both input forms, with the run merge on every level (NSIM_DEDUP_MAX_RES unset) and on none ("0")"""
    cfg, lv = _lotd()
    sset = _lotd_set(name)
    _margin_ok(sr.lotd_margin(lv), sset)
    dh, g, gn = _upstream(lv.num_levels, sset.S, 1)
    c = sr.lotd_contribs(lv, sset.points(form), dh.double(), _q(g, gn))
    for dedup in (None, "0"):
        if dedup is None:
            monkeypatch.delenv("NSIM_DEDUP_MAX_RES", raising=False)
        else:
            monkeypatch.setenv("NSIM_DEDUP_MAX_RES", dedup)
        _accept(_lotd_scatter(backend, cfg, sset, form, dh, g, gn), c, "nsim_lotd_scatter", backend)


def test_dense_ray_changes_cell_on_fine_levels_only():
    """what makes set 3 the parity-slot case: the cell never changes on the coarsest level and several times on the finest"""
    lv = _lotd()[1]
    p = _lotd_set("ray200").points("x")
    changes = []
    for l in (0, lv.num_levels - 1):
        c0 = torch.floor((p * 0.5 + 0.5) * (lv.res3[l][0] - 1.0))
        changes.append(int((c0[1:] != c0[:-1]).any(-1).sum()))
    assert changes[0] == 0 and changes[1] >= 3, changes


@pytest.mark.parametrize("form", ["x", "rays"])
def test_lotd_scatter_gn_null(backend, form):
    """gn = NULL: the first-order gradient.  g_planes is still required (code 28) and still READ -- include/nsim.h: it must be
    readable and finite; fields/nerf.py passes dh in its place -- so two different finite g_planes both meet the bound"""
    cfg, lv = _lotd()
    sset = _lotd_set("staggered")
    dh, g, _ = _upstream(lv.num_levels, sset.S, 2)
    c = sr.lotd_contribs(lv, sset.points(form), dh.double(), None)
    for g_pl in (dh, g * 1e6):
        _accept(_lotd_scatter(backend, cfg, sset, form, dh, g_pl, None), c, "nsim_lotd_scatter", backend)
    dgrid = torch.zeros(cfg.n_params, dtype=torch.float32, device=backend)
    with pytest.raises(RuntimeError, match="code 28"):
        _lib.call("nsim_lotd_scatter", cfg.meta, _lib.ptr(_dv(sset.x32(), backend)), None, None, None, None, None, sset.S,
                  _lib.ptr(_dv(dh, backend)), None, None, _lib.ptr(dgrid), 0, 0)
    _sync(backend)
    assert not bool(dgrid.any())


@pytest.mark.parametrize("name", ["staggered", "ray200"])
def test_lotd_scatter_level_halves(backend, name):
    """level_begin / level_count: the two halves into one dgrid are the full range; both meet the bound, and a half alone
    leaves the other half's levels at exactly 0.0"""
    cfg, lv = _lotd()
    sset = _lotd_set(name)
    L = lv.num_levels
    dh, g, gn = _upstream(L, sset.S, 3)
    c = sr.lotd_contribs(lv, sset.points("rays"), dh.double(), _q(g, gn))
    _accept(_lotd_scatter(backend, cfg, sset, "rays", dh, g, gn, begin=0, count=L), c, "nsim_lotd_scatter", backend)
    first = _lotd_scatter(backend, cfg, sset, "rays", dh, g, gn, begin=0, count=L // 2)
    _accept(first, sr.lotd_contribs(lv, sset.points("rays"), dh.double(), _q(g, gn), levels=range(L // 2)), "nsim_lotd_scatter",
            backend)
    both = _lotd_scatter(backend, cfg, sset, "rays", dh, g, gn, begin=L // 2, count=L - L // 2, dgrid=first.clone())
    _accept(both, c, "nsim_lotd_scatter", backend)
    with pytest.raises(RuntimeError, match="code 12"):
        _lotd_scatter(backend, cfg, sset, "rays", dh, g, gn, begin=L // 2, count=L)


@pytest.mark.parametrize("n_active", [1, 4, 9])
def test_lotd_scatter_active_levels(backend, n_active):
    """n_active_levels: the masked levels get exactly 0.0 (their entries are untouched in the list), the others the bound"""
    cfg, lv = _fresh_lotd()
    cfg.set_active_levels(n_active)
    sset = _lotd_set("ray200")
    dh, g, gn = _upstream(lv.num_levels, sset.S, 4)
    c = sr.lotd_contribs(lv, sset.points("x"), dh.double(), _q(g, gn), levels=range(n_active))
    got = _lotd_scatter(backend, cfg, sset, "x", dh, g, gn)
    _accept(got, c, "nsim_lotd_scatter", backend)
    assert not bool(got[lv.offsets[n_active]:].any())


@pytest.mark.parametrize("form", ["x", "rays"])
@pytest.mark.parametrize("name", ["staggered", "ray200"])
def test_lotd_scatter_cuboid_aabb(backend, name, form):
    """a cuboid pyramid over an AABB: per-axis vertex counts and x_scale / x_shift (1/3 is not a dyadic scale)"""
    cfg, lv = _lotd("cuboid")
    sset = _lotd_set(name, "cuboid")
    _margin_ok(sr.lotd_margin(lv), sset)
    dh, g, gn = _upstream(lv.num_levels, sset.S, 5)
    c = sr.lotd_contribs(lv, sset.points(form), dh.double(), _q(g, gn))
    _accept(_lotd_scatter(backend, cfg, sset, form, dh, g, gn), c, "nsim_lotd_scatter", backend)


@pytest.mark.parametrize("form", ["x", "rays"])
def test_lotd_scatter_lattice_points(backend, form):
    """set 6: points ON the cell decisions (w = 0, w = 1, the c0 = R - 2 clamp at u = 1), where f32 is exact"""
    cfg, lv = _lotd("lattice")
    sset = sr.lattice_points()
    for l in range(lv.num_levels):                       # exactness: the f32 evaluation of pos IS the f64 one
        pos32 = (sset.x32() * 0.5 + 0.5) * float(lv.res3[l][0] - 1)
        assert torch.equal(pos32.double(), (sset.points(form) * 0.5 + 0.5) * (lv.res3[l][0] - 1.0))
        assert bool((pos32 == pos32.round()).any()) and bool((pos32 == lv.res3[l][0] - 1.0).any())
    dh, g, gn = _upstream(lv.num_levels, sset.S, 6)
    c = sr.lotd_contribs(lv, sset.points(form), dh.double(), _q(g, gn))
    _accept(_lotd_scatter(backend, cfg, sset, form, dh, g, gn), c, "nsim_lotd_scatter", backend)


@pytest.mark.parametrize("name", ["staggered", "ray200", "interleaved128"])
def test_lotd_scatter_tiny_hash_table(backend, name):
    """set 7: 16-entry tables -- distinct vertices of one cell share an entry, and keys of DIFFERENT vertices on neighbouring
    lanes are equal: the merge folds them, legally (same address)"""
    cfg, lv = _lotd("tiny")
    sset = _lotd_set(name, "tiny")
    _margin_ok(sr.lotd_margin(lv), sset)
    dh, g, gn = _upstream(lv.num_levels, sset.S, 7)
    c = sr.lotd_contribs(lv, sset.points("x"), dh.double(), _q(g, gn))
    pairs = torch.unique(c.entry * sset.S + c.sample)         # vertices of ONE cell share an entry
    assert pairs.numel() < c.entry.numel()
    _accept(_lotd_scatter(backend, cfg, sset, "x", dh, g, gn), c, "nsim_lotd_scatter", backend)


@pytest.mark.parametrize("form", ["x", "rays"])
def test_lotd_scatter_batched_instances(backend, form):
    """set 8: two instances alternate lane by lane inside the same cell; the instance tables are whole pyramids at ray_goff
    (the kernel offsets the VERTEX by ray_goff >> 1, which also keeps the two instances' keys from merging)"""
    cfg, lv = _lotd()
    sset = _lotd_set("batched")
    _margin_ok(sr.lotd_margin(lv), sset)
    p = sset.points("x")
    for l in range(lv.num_levels):                       # neighbouring lanes (other instance) sit in the same cell
        c0 = torch.floor((p * 0.5 + 0.5) * (lv.res3[l][0] - 1.0))
        assert int((c0[1:] == c0[:-1]).all(-1).sum()) >= sset.S // 2
    goff = torch.tensor([0, cfg.n_params], dtype=torch.long)
    dh, g, gn = _upstream(lv.num_levels, sset.S, 8)
    c = sr.lotd_contribs(lv, sset.points(form), dh.double(), _q(g, gn), goff=goff[sset.ridx], n_entries=2 * cfg.n_params)
    got = _lotd_scatter(backend, cfg, sset, form, dh, g, gn, goff=goff, n_entries=2 * cfg.n_params)
    _accept(got, c, "nsim_lotd_scatter", backend)
    assert bool(got[:cfg.n_params].any()) and bool(got[cfg.n_params:].any())


def test_lotd_scatter_no_samples(backend):
    cfg, lv = _lotd()
    dgrid = torch.zeros(cfg.n_params, dtype=torch.float32, device=backend)
    e = torch.zeros(0, dtype=torch.float32, device=backend)
    _lib.call("nsim_lotd_scatter", cfg.meta, _lib.ptr(e), None, None, None, None, None, 0, _lib.ptr(e), _lib.ptr(e), None,
              _lib.ptr(dgrid), 0, 0)
    _sync(backend)
    assert not bool(dgrid.any())


_POOL = 5


@settings(**SET)
@given(runs=st.lists(st.tuples(st.integers(0, _POOL - 1), st.sampled_from([1, 1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 33, 64, 65, 70])),
                     min_size=1, max_size=14),
       dedup=st.booleans(), seed=st.integers(0, 10 ** 6))
def test_lotd_and_permuto_scatter_random_runs(backend, monkeypatch, runs, dedup, seed):
    """set 9: random compositions of run lengths in random orders over a pool of five points (two neighbouring runs may name
    the same point: one longer run)"""
    total = 0
    runs = [r for r in runs if (total := total + r[1]) <= 512]
    cfg, lv = _lotd()
    sset = sr.from_runs("random", [r[0] for r in runs], [r[1] for r in runs], n_pool=_POOL, margin_fn=sr.lotd_margin(lv), seed=21)
    dh, g, gn = _upstream(lv.num_levels, sset.S, seed)
    if dedup:
        monkeypatch.delenv("NSIM_DEDUP_MAX_RES", raising=False)
    else:
        monkeypatch.setenv("NSIM_DEDUP_MAX_RES", "0")
    c = sr.lotd_contribs(lv, sset.points("rays"), dh.double(), _q(g, gn))
    _accept(_lotd_scatter(backend, cfg, sset, "rays", dh, g, gn), c, "nsim_lotd_scatter", backend)
    pc, pm = _permuto(3)
    pset = sr.from_runs("random", [r[0] for r in runs], [r[1] for r in runs], n_pool=_POOL, margin_fn=sr.permuto_margin(pm), seed=21)
    dh, g, gn = _upstream(pm.num_levels, pset.S, seed + 1)
    cp = sr.permuto_contribs(pm, pset.points("rays"), dh.double(), g.double(), gn.double())
    _accept(_permuto_scatter(backend, pc, pset, "rays", None, dh, g, gn), cp, "nsim_permuto_scatter", backend)


# =================================================================================================== nsim_lotd4_scatter
@functools.lru_cache(maxsize=None)
def _lotd4():
    res_xyz, res_w, T = [3, 4, 6, 9, 17, 40], [2, 3, 4, 7, 12, 30], 2 ** 9
    types, sizes, offs, off = [], [], [], 0
    for rx, rw in zip(res_xyz, res_w):
        n = rx ** 3 * rw
        types.append("Dense" if n <= T else "Hash")
        sizes.append(n if n <= T else T)
        offs.append(off)
        off += sizes[-1] * 2
    spec = odist.LoTD4Spec(res_xyz, res_w, types, sizes, offs, off, T)
    m = _lib.Lotd4Meta()
    m.num_levels = spec.num_levels
    for l in range(spec.num_levels):
        m.res_xyz[l], m.res_w[l], m.type[l] = res_xyz[l], res_w[l], 0 if types[l] == "Dense" else 1
        m.size[l], m.offset[l] = sizes[l], offs[l]
    return spec, m


@functools.lru_cache(maxsize=None)
def _lotd4_set(name):
    kw = dict(dim=4, box=(0.0, 1.0), margin_fn=sr.lotd4_margin(_lotd4()[0]))
    if name.startswith("identical"):
        return sr.identical(int(name[9:]), **kw)
    if name == "staggered":
        return sr.staggered(**kw)
    if name == "holes":
        return sr.holes(200, **kw)
    return sr.dense_ray(int(name[3:]), **kw)


def _lotd4_scatter(device, meta, n_params, u4, valid, dh):
    dgrid = torch.zeros(n_params, dtype=torch.float32, device=device)
    _lib.call("nsim_lotd4_scatter", meta, _lib.ptr(_dv(u4, device)), _lib.ptr(_dv(valid.to(torch.uint8), device)), u4.shape[0],
              _lib.ptr(_dv(dh, device)), _lib.ptr(dgrid))
    _sync(device)
    return dgrid


@pytest.mark.parametrize("name", [f"identical{S}" for S in sr.IDENTICAL_S] + ["staggered", "ray64", "ray200", "holes"])
def test_lotd4_scatter_sets(backend, name):
    """the 4-D scatter (16 corners, parity slots over four axes); with holes the skipped samples' dh rows are NaN"""
    spec, meta = _lotd4()
    sset = _lotd4_set(name)
    _margin_ok(sr.lotd4_margin(spec), sset)
    dh = _upstream(spec.num_levels, sset.S, 11)[0]
    c = sr.lotd4_contribs(spec, sset.points("x"), dh.double())
    c = c.select(sset.valid[c.sample])
    dh_dev = dh.clone()
    dh_dev[:, ~sset.valid] = float("nan")
    assert name != "holes" or int((~sset.valid).sum()) > 60
    _accept(_lotd4_scatter(backend, meta, spec.n_params, sset.x32(), sset.valid, dh_dev), c, "nsim_lotd4_scatter", backend)


def test_lotd4_scatter_nothing_valid(backend):
    """valid all zero writes nothing (dh NaN-poisoned); S = 0 returns 0 and writes nothing"""
    spec, meta = _lotd4()
    sset = _lotd4_set("ray200")
    dh = torch.full((spec.num_levels, sset.S, 2), float("nan"))
    got = _lotd4_scatter(backend, meta, spec.n_params, sset.x32(), torch.zeros(sset.S, dtype=torch.bool), dh)
    assert not bool(got.any())
    got = _lotd4_scatter(backend, meta, spec.n_params, torch.zeros(0, 4), torch.zeros(0, dtype=torch.bool), torch.zeros(0))
    assert not bool(got.any())


# =================================================================================================== permutohedral lattice
@functools.lru_cache(maxsize=None)
def _permuto(D, log2_T=10):
    pc = PermutoConfig(in_dim=D, n_levels=6, n_feats=2, log2_hashmap_size=log2_T, coarsest_res=1.5, finest_res=160.0, seed=3)
    return pc, sr.permuto_levels(pc)


def _z(D, sset):
    """the per-ray condition of a conditioned field (in_dim = D > 3)"""
    g = torch.Generator().manual_seed(40 + D)
    return torch.rand(int(sset.o.shape[0]), D - 3, generator=g) * 2 - 1


@functools.lru_cache(maxsize=None)
def _permuto_set(name, D, pointwise=False):
    """pointwise: a D-dimensional set (standalone / point-mode kernels); else a 3-D set whose rays carry a condition"""
    pm = _permuto(D)[1]
    if pointwise:
        kw = dict(dim=D, margin_fn=sr.permuto_margin(pm))
    elif D == 3:
        kw = dict(margin_fn=sr.permuto_margin(pm))
    else:
        n_rays = {"staggered": 7, "interleaved128": 2}.get(name, 1)
        g = torch.Generator().manual_seed(40 + D)
        kw = dict(margin_fn=sr.permuto_margin(pm, torch.rand(n_rays, D - 3, generator=g) * 2 - 1))
    if name.startswith("identical"):
        return sr.identical(int(name[9:]), **kw)
    if name == "staggered":
        return sr.staggered(**kw)
    if name == "holes":
        return sr.holes(200, **kw)
    if name.startswith("interleaved"):
        return sr.interleaved(int(name[11:]), **kw)
    return sr.dense_ray(int(name[3:]), **kw)


@pytest.mark.parametrize("name", ["identical1", "identical63", "identical64", "identical65", "identical130", "staggered", "ray200"])
@pytest.mark.parametrize("D", [3, 4, 7])
def test_permuto_bwd_sets(backend, D, name):
    """the standalone backward (dL/dout point-major), runs keyed by the vertex"""
    pc, pm = _permuto(D)
    sset = _permuto_set(name, D, True)
    _margin_ok(sr.permuto_margin(pm), sset)
    S, L = sset.S, pm.num_levels
    dh = _upstream(L, S, 12)[0]
    c = sr.permuto_contribs(pm, sset.points("x"), dh.double())
    dgrid = torch.zeros(pm.n_params, dtype=torch.float32, device=backend)
    _lib.call("nsim_permuto_bwd", pc.meta, _lib.ptr(_dv(sset.x32(), backend)), S,
              _lib.ptr(_dv(dh.permute(1, 0, 2).reshape(S, 2 * L), backend)), _lib.ptr(dgrid))
    _sync(backend)
    _accept(dgrid, c, "nsim_permuto_bwd", backend)


def _permuto_scatter(device, pc, sset, form, z, dh, g, gn):
    dgrid = torch.zeros(pc.n_params, dtype=torch.float32, device=device)
    if form == "x":
        x, o, d, t = _dv(sset.x32(), device), None, None, None
        ridx = _dv(sset.ridx, device) if z is not None else None
    else:
        x, o, d, t, ridx = None, _dv(sset.o, device), _dv(sset.d, device), _dv(sset.t, device), _dv(sset.ridx, device)
    _lib.call("nsim_permuto_scatter", pc.meta, _lib.ptr(x), _lib.ptr(o), _lib.ptr(d), _lib.ptr(t), _lib.ptr(ridx),
              _lib.ptr(_dv(z, device)), sset.S, _lib.ptr(_dv(dh, device)), _lib.ptr(_dv(g, device)), _lib.ptr(_dv(gn, device)),
              _lib.ptr(dgrid))
    _sync(device)
    return dgrid


@pytest.mark.parametrize("second", [True, False])
@pytest.mark.parametrize("form", ["x", "rays"])
@pytest.mark.parametrize("name", ["identical65", "staggered", "ray200", "interleaved128"])
@pytest.mark.parametrize("D", [3, 5])
def test_permuto_scatter_sets(backend, D, name, form, second):
    """the field's scatter: positions or rays, in_dim = 5 with the per-ray condition z, gn given (second-order term) and NULL
    (then g_planes may be NULL too)"""
    pc, pm = _permuto(D)
    sset = _permuto_set(name, D)
    z = None if D == 3 else _z(D, sset)
    _margin_ok(sr.permuto_margin(pm, z), sset)
    p = sset.points(form) if z is None else torch.cat([sset.points(form), z.double()[sset.ridx]], dim=1)
    dh, g, gn = _upstream(pm.num_levels, sset.S, 13)
    if second:
        c = sr.permuto_contribs(pm, p, dh.double(), g.double(), gn.double())
        got = _permuto_scatter(backend, pc, sset, form, z, dh, g, gn)
    else:
        c = sr.permuto_contribs(pm, p, dh.double())
        got = _permuto_scatter(backend, pc, sset, form, z, dh, None, None)
    _accept(got, c, "nsim_permuto_scatter", backend)


@pytest.mark.parametrize("name", ["staggered", "ray200"])
def test_permuto_scatter_tiny_hash_table(backend, name):
    """set 7 on the lattice: 16 entries per level -- the d + 1 vertices of a simplex collide, neighbouring lanes' different
    vertices share keys (the lattice arithmetic does not depend on T: the sets and their margin are those of T = 2^10)"""
    pc, pm = _permuto(3, 4)
    sset = _permuto_set(name, 3)
    _margin_ok(sr.permuto_margin(pm), sset)
    dh, g, gn = _upstream(pm.num_levels, sset.S, 18)
    c = sr.permuto_contribs(pm, sset.points("rays"), dh.double(), g.double(), gn.double())
    _accept(_permuto_scatter(backend, pc, sset, "rays", None, dh, g, gn), c, "nsim_permuto_scatter", backend)


@pytest.mark.parametrize("name", ["identical65", "staggered", "ray200", "holes"])
def test_permuto_scatter_pts_sets(backend, name):
    """the point-mode scatter on a 4-D lattice with a valid mask: skipped points' dh rows are NaN"""
    pc, pm = _permuto(4)
    sset = _permuto_set(name, 4, True)
    _margin_ok(sr.permuto_margin(pm), sset)
    dh = _upstream(pm.num_levels, sset.S, 14)[0]
    c = sr.permuto_contribs(pm, sset.points("x"), dh.double())
    c = c.select(sset.valid[c.sample])
    dh_dev = torch.full((16, sset.S, 2), float("nan"))
    dh_dev[:pm.num_levels] = dh
    dh_dev[:, ~sset.valid] = float("nan")
    dgrid = torch.zeros(pm.n_params, dtype=torch.float32, device=backend)
    _lib.call("nsim_permuto_scatter_pts", pc.meta, _lib.ptr(_dv(sset.x32(), backend)),
              _lib.ptr(_dv(sset.valid.to(torch.uint8), backend)), sset.S, _lib.ptr(_dv(dh_dev, backend)), _lib.ptr(dgrid))
    _sync(backend)
    _accept(dgrid, c, "nsim_permuto_scatter_pts", backend)


def test_permuto_scatter_pts_nothing_valid(backend):
    pc, pm = _permuto(4)
    sset = _permuto_set("ray200", 4, True)
    dgrid = torch.zeros(pm.n_params, dtype=torch.float32, device=backend)
    nan = _dv(torch.full((16, sset.S, 2), float("nan")), backend)
    _lib.call("nsim_permuto_scatter_pts", pc.meta, _lib.ptr(_dv(sset.x32(), backend)),
              _lib.ptr(torch.zeros(sset.S, dtype=torch.uint8, device=backend)), sset.S, _lib.ptr(nan), _lib.ptr(dgrid))
    e = torch.zeros(0, dtype=torch.float32, device=backend)
    _lib.call("nsim_permuto_scatter_pts", pc.meta, _lib.ptr(e), _lib.ptr(torch.zeros(0, dtype=torch.uint8, device=backend)), 0,
              _lib.ptr(e), _lib.ptr(dgrid))
    _sync(backend)
    assert not bool(dgrid.any())


@pytest.mark.parametrize("form", ["x", "rays"])
@pytest.mark.parametrize("name", ["identical130", "staggered", "ray200", "interleaved128"])
def test_permuto_dz_sets(backend, name, form):
    """d L / d z: runs keyed by the RAY -- one run of 64 per wave on a single ray, the staggered runs over seven rays, no run
    at all with two rays interleaved (every lane its own atomic on one of two addresses)"""
    D = 5
    pc, pm = _permuto(D)
    sset = _permuto_set(name, D)
    z = _z(D, sset)
    _margin_ok(sr.permuto_margin(pm, z), sset)
    R = int(sset.o.shape[0])
    p = torch.cat([sset.points(form), z.double()[sset.ridx]], dim=1)
    g = torch.Generator().manual_seed(15)
    table = torch.randn(pm.n_params, generator=g).half()
    dh = _upstream(pm.num_levels, sset.S, 15)[0]
    c = sr.permuto_dz_contribs(pm, table, p, sset.ridx, R, dh.double())
    dz = torch.zeros(R, D - 3, dtype=torch.float32, device=backend)
    if form == "x":
        x, o, d, t = _dv(sset.x32(), backend), None, None, None
    else:
        x, o, d, t = None, _dv(sset.o, backend), _dv(sset.d, backend), _dv(sset.t, backend)
    _lib.call("nsim_permuto_dz", pc.meta, _lib.ptr(_dv(table, backend)), _lib.ptr(x), _lib.ptr(o), _lib.ptr(d), _lib.ptr(t),
              _lib.ptr(_dv(sset.ridx, backend)), _lib.ptr(_dv(z, backend)), sset.S, _lib.ptr(_dv(dh, backend)), _lib.ptr(dz))
    _sync(backend)
    _accept(dz, c, "nsim_permuto_dz", backend, per_term=True)


# =================================================================================================== the controls
@pytest.mark.parametrize("second", [True, False])
@pytest.mark.parametrize("name", ["staggered", "ray200"])
def test_lotd_bwd_control(backend, name, second):
    """nsim_lotd_bwd has no merge (one atomic per corner and feature): the same sets, the same lists, the same bound"""
    cfg, lv = _lotd()
    sset = _lotd_set(name)
    S, L = sset.S, lv.num_levels
    g = torch.Generator().manual_seed(16)
    dout = torch.randn(S, 2 * L, generator=g)
    ddydx = torch.randn(S, 2 * L, 3, generator=g) if second else None
    dh = dout.view(S, L, 2).permute(1, 0, 2)
    q = ddydx.view(S, L, 2, 3).permute(1, 0, 2, 3).double() if second else None
    c = sr.lotd_contribs(lv, sset.points("x"), dh.double(), q)
    dgrid = torch.zeros(cfg.n_params, dtype=torch.float32, device=backend)
    _lib.call("nsim_lotd_bwd", _lib.ptr(_dv(sset.x32(), backend)), _lib.ptr(_dv(dout, backend)), _lib.ptr(_dv(ddydx, backend)),
              cfg.meta, S, _lib.ptr(dgrid))
    _sync(backend)
    _accept(dgrid, c, "nsim_lotd_bwd", backend)


@pytest.mark.parametrize("with_dv", [True, False])
@pytest.mark.parametrize("name", ["identical257", "staggered", "ray200", "interleaved128"])
def test_ray_grad_reduce(backend, name, with_dv):
    """d_rays_o[r] += dx_s, d_rays_d[r] += t_s dx_s + dv_s against ``index_add`` in f64: up to 256 atomics of a block on three
    addresses"""
    sset = _lotd_set(name)
    S, R = sset.S, int(sset.o.shape[0])
    g = torch.Generator().manual_seed(17)
    dx, dv = torch.randn(S, 3, generator=g), (torch.randn(S, 3, generator=g) if with_dv else None)
    t = torch.rand(S, generator=g) * 4
    co, cd = sr.ray_reduce_contribs(dx.double(), None if dv is None else dv.double(), t.double(), sset.ridx, R)
    ref_o = torch.zeros(R, 3, dtype=F64).index_add_(0, sset.ridx, dx.double())
    assert torch.equal(co.gradient().view(R, 3), ref_o)
    d_o = torch.zeros(R, 3, dtype=torch.float32, device=backend)
    d_d = torch.zeros(R, 3, dtype=torch.float32, device=backend)
    _lib.call("nsim_ray_grad_reduce", _lib.ptr(_dv(dx, backend)), _lib.ptr(_dv(dv, backend)), _lib.ptr(_dv(t, backend)),
              _lib.ptr(_dv(sset.ridx, backend)), S, _lib.ptr(d_o), _lib.ptr(d_d))
    _sync(backend)
    _accept(d_o, co, "nsim_ray_grad_reduce", backend, per_term=True)
    _accept(d_d, cd, "nsim_ray_grad_reduce", backend, per_term=True)
