"""Dynamic-only EmerNeRF street model (fg_neus=permuto_emernerf/with_gtbox.240212.yaml, ``Dynamic``): the fused decoders of
csrc/nerf_field.hip (nsim_dyn_fwd / nsim_dyn_bwd), the time input, the time-sliced density occupancy grid and the host model
(neuralsim_amd/fields/dynamic_nerf.py) against the float64 restatement tests/dynamic_nerf_ref.py."""
import copy
from pathlib import Path

import pytest
import torch

import dynamic_nerf_ref as dr
import ref_glue
from oracle import render as orr
from util import leaf, rel_l2

AABB = torch.tensor([[-2.0, -1, -1], [2.0, 1, 1]])       # dyadic centre / half-extent: the folded lattice scale is exact
STEP, MAX_STEPS = 0.11, 64
GOLDEN = Path(__file__).resolve().parent / "golden" / "emernerf_dynamic_model_params.yaml"
REF_YAML = Path("/root/reference/code_multi/configs/exps/fg_neus=permuto_emernerf/with_gtbox.240212.yaml")


def yaml_params(levels=6, log2T=10, n_appear=0, dtype="float", res=(8, 4, 4), **over):
    """The ``model_params`` block of with_gtbox.240212.yaml:279-360 with the sizes overridden down."""
    p = dict(
        dtype=dtype, n_geometry_feat=64, n_semantic_feat=0,
        time_embedding_cfg=dict(dim=1, learnable=False, weight_init=dict(type="linspace", start=-1, end=1)),
        dynamic_encoding_cfg=dict(type="permuto", param=dict(permuto_auto_compute_cfg=dict(
            type="multi_res", coarsest_res=4.0, finest_res=32.0, n_levels=levels, n_feats=2, log2_hashmap_size=log2T,
            apply_random_shifts_per_level=True))),
        dynamic_decoder_cfg=dict(type="mlp", D=1, W=64, activation="relu"),
        use_flow_field=False, use_shadow=False,
        radiance_cfg=dict(use_pos=False, use_nablas=False, use_view_dirs=True, D=2, W=64, dir_embed_cfg=dict(type="spherical", degree=4),
                          n_appear_embedding=n_appear),
        accel_cfg=dict(type="occ_grid_dynamic", resolution=list(res), occ_thre_consider_mean=True, occ_thre=0.5, ema_decay=0.95,
                       init_cfg=dict(mode="constant", constant_value=1.0e-2), update_from_net_cfg=dict(num_steps=1, num_pts=512),
                       update_from_samples_cfg={}, n_steps_between_update=16, n_steps_warmup=256),
        ray_query_cfg=dict(query_mode="march_occ", query_param=dict(march_cfg=dict(step_size=STEP, max_steps=MAX_STEPS))))
    p.update(over)
    return p


def keyframes(T):
    return torch.arange(T, dtype=torch.float32) * 0.25       # 0, 0.25, ...: keyframes and midpoints are exact in f32


def pattern(K, res):
    """hand-set occupancy per slice: the voxels with (i + j + k + slice) % 3 == 0, storage order x fastest -> bool [K, nvox]"""
    v = torch.arange(res[0] * res[1] * res[2])
    i, j, k = v % res[0], (v // res[0]) % res[1], v // (res[0] * res[1])
    return torch.stack([(i + j + k + s) % 3 == 0 for s in range(K)])


def build(backend, levels=6, log2T=10, n_appear=0, precision="f32", seed=11, T=5, n_jump=2, res=(8, 4, 4)):
    from neuralsim_amd.fields.dynamic_nerf import EmerNeRFOnlyDynamicModel
    m = EmerNeRFOnlyDynamicModel(**yaml_params(levels, log2T, n_appear, dtype={"f32": "float", "fp16": "half"}[precision], res=res))
    ts = keyframes(T)
    m.populate(aabb=AABB, ts_keyframes=ts, accel_n_jump_frames=n_jump)
    p = dr.make_dyn_params(ts, AABB, levels, log2T, 4.0, 32.0, n_appear, seed=seed)
    assert p.spec.n_params == m.encoding.cfg.n_params and m.accel.K == len(ts[::n_jump])
    with torch.no_grad():
        m.encoding.flattened_params.copy_(p.grid.float())
        m.den_w.copy_(torch.cat([w.reshape(-1) for w in p.den_w]).float())
        m.den_b.copy_(torch.cat(p.den_b).float())
        m.rad_w.copy_(torch.cat([w.reshape(-1) for w in p.rad_w]).float())
        m.rad_b.copy_(torch.cat(p.rad_b).float())
    m = m.to(backend)
    occ = pattern(m.accel.K, res)
    m.accel.occ_val.copy_(occ.float().reshape(-1).to(backend))
    m.accel.pack_bits()
    return m, p, occ


_RAYS = {}


def rays(R):
    """R rays from outside the box towards points inside it, every fourth shifted to miss it; times on keyframes, midpoints,
    off-grid values and outside the range.  Computed once per R."""
    if R not in _RAYS:
        g = torch.Generator().manual_seed(100 + R)
        o = torch.tensor([-3.5, 0.0, 0.0]) + (torch.rand(R, 3, generator=g) - 0.5) * torch.tensor([0.5, 1.0, 1.0])
        tgt = (torch.rand(R, 3, generator=g) - 0.5) * torch.tensor([3.0, 1.5, 1.5])
        d = tgt - o
        d = d / d.norm(dim=-1, keepdim=True) * (0.8 + 0.4 * torch.rand(R, 1, generator=g))     # not normalised
        if R > 1:
            o[3::4] += torch.tensor([0.0, 5.0, 0.0])
        cand = torch.tensor([0.0, 0.125, 0.25, 0.3125, 0.5, 0.75, 0.875, 1.0, -0.5, 1.75, 0.625])
        ts = cand[torch.randint(0, cand.numel(), (R,), generator=g)]
        near, far, hit = orr.aabb_ray_test(o, d, AABB[0], AABB[1], 0.01, None)
        _RAYS[R] = dict(o=o, d=d, ts=ts, near=near, far=far, hit=hit, ha=torch.randn(R, 4, generator=g) * 0.3)
    return _RAYS[R]


def run_query(m, backend, R, ha=None, ts=None, **cfg):
    r = rays(R)
    dv = lambda t: t.to(backend).contiguous()      # noqa: E731
    kw = dict(rays_h_appear=ha) if ha is not None else {}
    tested = m.ray_test(dv(r["o"]), dv(r["d"]), near=0.01, rays_ts=dv(r["ts"] if ts is None else ts), **kw)
    return tested, m.ray_query(ray_tested=tested, config=dict(cfg), return_details=True)


def ref_march(m, r, occ, res, jitter=None):
    """The restatement's samples of the hit rays of ``r`` on the per-slice occupancy ``occ``."""
    hit = r["hit"]
    sl = dr.slice_of(m.accel.ts_keyframes.cpu(), r["ts"][hit])
    jit = torch.zeros(int(hit.sum())) if jitter is None else jitter
    return dr.march_sliced(r["o"][hit], r["d"][hit], r["near"][hit], r["far"][hit], jit, sl, occ, AABB, list(res), STEP, MAX_STEPS), sl


def flat_grads(p):
    return dict(grid=p.grid.grad, den_w=torch.cat([w.grad.reshape(-1) for w in p.den_w]), den_b=torch.cat([b.grad for b in p.den_b]),
                rad_w=torch.cat([w.grad.reshape(-1) for w in p.rad_w]), rad_b=torch.cat([b.grad for b in p.rad_b]))


# ------------------------------------------------------------------------------------------------ 1. decoder parity
def points(S, R=5, seed=3):
    g = torch.Generator().manual_seed(seed + S)
    x = (torch.rand(S, 3, generator=g) - 0.5) * torch.tensor([3.9, 1.9, 1.9])
    ridx = torch.sort(torch.randint(0, R, (S,), generator=g)).values
    d = torch.randn(R, 3, generator=g)
    ts = torch.rand(R, generator=g) * 1.2 - 0.1
    return dict(x=x, ridx=ridx, d=d, ts=ts, ha=torch.randn(R, 4, generator=g) * 0.3, ws=torch.randn(S, generator=g) * 0.1,
                wa=torch.randn(S, generator=g), wr=torch.randn(S, 3, generator=g))


def decode(m, backend, q, ha=None, with_rgb=True):
    """The model's gather + decoders at explicit samples (x [S,3], a ray index per sample, per-ray direction / time / code)."""
    from neuralsim_amd.fields.dynamic_nerf import _DynFn
    dv = lambda t: t.to(backend).contiguous()      # noqa: E731
    S = q["x"].shape[0]
    w = m.time_coord(dv(q["ts"][q["ridx"]]))
    x4 = m._points(w, S, x=dv(q["x"]))
    return _DynFn.apply(m, m.encoding.flattened_params, m.den_w, m.den_b, m.rad_w, m.rad_b, ha, x4, dv(q["d"]), dv(q["ridx"]),
                        STEP, with_rgb)


def value_errors(got, ref):
    sg, al, rgb = got
    return dict(sigma=float((sg.detach().cpu() - ref["sigma"].detach()).abs().max()) / (1 + float(ref["sigma"].detach().max())),
                alpha=float((al.detach().cpu() - ref["opacity_alpha"].detach()).abs().max()),
                rgb=float((rgb.detach().cpu() - ref["rgb"].detach()).abs().max()))


PARITY = [(1, 6, 10, 0), (31, 6, 10, 4), (32, 1, 10, 0), (33, 6, 4, 4), (257, 6, 10, 4), (257, 16, 10, 0), (33, 16, 4, 4)]


@pytest.mark.parametrize("S,levels,log2T,n_appear", PARITY)
@pytest.mark.parametrize("precision", ["f32", "fp16"])
def test_decoder_parity(backend, precision, S, levels, log2T, n_appear):
    """sigma / alpha / rgb and every gradient at given samples against the float64 restatement.  Bounds: those of
    tests/test_nerf.py::test_decoder_parity for this decoder family (values 2e-5 | 5e-3, alpha ten times that; gradients 3e-4 |
    6.24e-2 rel-L2).  The wider fp16 layers of this model (64 geometry rows, an 84-wide radiance input) stay inside them:
    measured values in DESIGN.md sec. 7."""
    m, p, _ = build(backend, levels, log2T, n_appear, precision)
    q = points(S)
    p.requires_grad_(True)
    ha_d = leaf(q["ha"], backend) if n_appear else None
    ha_o = leaf(q["ha"], dtype=torch.float64) if n_appear else None
    got = decode(m, backend, q, ha_d)
    ref = dr.query_points(p, q["x"], q["ts"][q["ridx"]], q["d"][q["ridx"]], ha_o[q["ridx"]] if n_appear else None, STEP)
    loss = lambda o: (o["sigma"] * q["ws"]).sum() + (o["opacity_alpha"] * q["wa"]).sum() + (o["rgb"] * q["wr"]).sum()   # noqa: E731
    loss(ref).backward()
    refg = flat_grads(p)
    if n_appear:
        refg["h_appear"] = ha_o.grad
    tol = dict(f32=2e-5, fp16=5e-3)[precision]
    vtol = dict(sigma=tol, rgb=tol, alpha=10 * tol)
    gtol = {k: dict(f32=3e-4, fp16=6.24e-2)[precision] for k in refg}
    ev = value_errors(got, ref)
    print(f"[dyn parity {precision} S={S} L={levels} T={log2T} na={n_appear}] values", {k: f"{v:.2e}" for k, v in ev.items()})
    for k, e in ev.items():
        assert e < vtol[k], (k, e, vtol[k])
    dvw = lambda t: t.to(backend)      # noqa: E731
    ((got[0] * dvw(q["ws"])).sum() + (got[1] * dvw(q["wa"])).sum() + (got[2] * dvw(q["wr"])).sum()).backward()
    gg = dict(grid=m.encoding.flattened_params.grad, den_w=m.den_w.grad, den_b=m.den_b.grad, rad_w=m.rad_w.grad, rad_b=m.rad_b.grad)
    if n_appear:
        gg["h_appear"] = ha_d.grad
    errs = {k: rel_l2(gg[k].cpu(), refg[k]) for k in refg}
    print(f"[dyn parity {precision} S={S} L={levels} T={log2T} na={n_appear}] grads", {k: f"{v:.2e}" for k, v in errs.items()})
    for k, e in errs.items():
        assert e < gtol[k], (k, e, gtol[k])


@pytest.mark.parametrize("precision", ["f32", "fp16"])
def test_density_only_path(backend, precision):
    """rgb not requested: the same sigma / alpha, gradients to the table and the dynamic decoder, None (not zeros) for the
    radiance decoder."""
    m, p, _ = build(backend, 6, 10, 4, precision)
    q = points(33)
    full = decode(m, backend, q, q["ha"].to(backend))
    dens = decode(m, backend, q, None, with_rgb=False)
    assert len(dens) == 2
    assert torch.equal(full[0].detach(), dens[0].detach()) and torch.equal(full[1].detach(), dens[1].detach())
    p.requires_grad_(True)
    ref = dr.query_points(p, q["x"], q["ts"][q["ridx"]], None, None, STEP)
    ((ref["sigma"] * q["ws"]).sum() + (ref["opacity_alpha"] * q["wa"]).sum()).backward()
    ((dens[0] * q["ws"].to(backend)).sum() + (dens[1] * q["wa"].to(backend)).sum()).backward()
    assert m.rad_w.grad is None and m.rad_b.grad is None
    gtol = dict(f32=3e-4, fp16=6.24e-2)[precision]
    # (the geometry rows of the second layer are no part of the density: exactly zero)
    assert float(m.den_w.grad[64 * 12 + 64:].abs().max()) == 0.0 and float(m.den_b.grad[65:].abs().max()) == 0.0
    refg = flat_grads_density(p)
    for k, g_ in dict(grid=m.encoding.flattened_params.grad, den_w=m.den_w.grad, den_b=m.den_b.grad).items():
        assert rel_l2(g_.cpu(), refg[k]) < gtol, k


def flat_grads_density(p):
    z = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)      # noqa: E731
    return dict(grid=z(p.grid), den_w=torch.cat([z(w).reshape(-1) for w in p.den_w]), den_b=torch.cat([z(b) for b in p.den_b]))


def test_weight_gradient_replicas(backend, monkeypatch):
    """The weight gradients through the replicas of the registered scratch equal the direct flush."""
    from neuralsim_amd import _lib
    grads = []
    q = points(257)
    for min_wg in ("1000000", "1"):
        monkeypatch.setenv("NSIM_GRAD_REPLICAS_MIN_WG", min_wg)
        m, _, _ = build(backend, 6, 10, 4, "f32")
        _lib.ensure_grad_scratch(backend)
        ha = leaf(q["ha"], backend)
        got = decode(m, backend, q, ha)
        (got[1].sum() + got[2].sum()).backward()
        grads.append([g_.grad.cpu().clone() for g_ in (m.den_w, m.den_b, m.rad_w, m.rad_b)])
    for a, b in zip(*grads):
        assert float(b.abs().sum()) > 0 and rel_l2(a, b) < 1e-5
    assert float(_lib.ensure_grad_scratch(backend).abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------ 2. softplus truncation
@pytest.mark.parametrize("raw", [-30.0, 0.0, 14.9, 15.1, 40.0])
def test_trunc_softplus(backend, raw):
    """A zero density row and a bias of ``raw`` give every sample that raw value: sigma = log1p(exp(raw)), and the gradient of
    sum(sigma) to that bias is S sigmoid(min(raw, 15))."""
    import math
    m, p, _ = build(backend, 6, 10, 0, "f32")
    F = 12
    with torch.no_grad():
        m.den_w[64 * F:64 * F + 64] = 0.0
        m.den_b[64] = raw
        p.den_w[1][0] = 0.0
        p.den_b[1][0] = raw
    S = 33
    q = points(S)
    x, ts = q["x"].to(backend), q["ts"][q["ridx"]].to(backend)
    sig = m.forward_density(x, ts)["sigma"]
    want = math.log1p(math.exp(raw))
    assert torch.allclose(sig.detach().cpu().double(), torch.full([S], want, dtype=torch.float64), rtol=1e-6, atol=1e-30)
    p.requires_grad_(True)
    ref = dr.query_points(p, q["x"], q["ts"][q["ridx"]])
    assert torch.allclose(ref["sigma"].detach(), torch.full([S], want, dtype=torch.float64), rtol=1e-12)
    ref["sigma"].sum().backward()
    sig.sum().backward()
    dsig = 1.0 / (1.0 + math.exp(-min(raw, 15.0)))
    assert abs(float(p.den_b[1].grad[0]) - S * dsig) < 1e-9 * S
    assert abs(float(m.den_b.grad[64]) - S * dsig) < 2e-6 * S * max(dsig, 1e-30) + 1e-30
    assert rel_l2(m.den_w.grad[64 * F:64 * F + 64].cpu(), p.den_w[1].grad[0]) < 3e-4


# ------------------------------------------------------------------------------------------------ 3. time input
@pytest.mark.parametrize("T,n_jump", [(5, 2), (5, 1), (3, 2), (1, 1), (1, 2)])
def test_time_coordinate_and_slice(backend, T, n_jump):
    """Keyframes, midpoints (a tie goes to the lower slice), times before and after the range, T == 1: the f32 kernel equals
    the float64 restatement exactly (keyframe times, codes and query times are dyadic, so both are exact)."""
    m, p, _ = build(backend, 1, 4, 0, "f32", T=T, n_jump=n_jump)
    tk = keyframes(T)
    ts = torch.cat([tk, (tk[1:] + tk[:-1]) * 0.5, tk + 0.0625, torch.tensor([-1.0, -0.125, float(tk[-1]) + 0.125, 7.0, 0.375])])
    if T in (3, 5):
        codes = p.codes
        assert torch.equal(codes, torch.linspace(-1, 1, T).double()) and torch.equal(m.time_codes.cpu().double(), codes)
    w = m.time_coord(ts.to(backend)).cpu()
    assert torch.equal(w.double(), dr.time_coord(p.ts_keyframes, p.codes, ts))
    assert float(w.min()) >= -1.0 and float(w.max()) <= 1.0
    acc = m.accel
    tsa = tk[::n_jump]
    assert torch.equal(acc.ts_keyframes.cpu(), tsa) and acc.K == tsa.numel()
    sl = acc.slice_of(ts.to(backend)).cpu()
    assert torch.equal(sl, dr.slice_of(tsa, ts))
    assert torch.equal(acc.ray_word_off(ts.to(backend)).cpu(), sl * acc.words_per_slice)
    if acc.K > 1:
        mid = (tsa[1:] + tsa[:-1]) * 0.5
        assert torch.equal(acc.slice_of(mid.to(backend)).cpu(), torch.arange(acc.K - 1))         # tie -> lower index
        assert int(sl[ts == -1.0]) == 0 and int(sl[ts == 7.0]) == acc.K - 1


# ------------------------------------------------------------------------------------------------ 4. sliced accelerator
@pytest.mark.parametrize("res", [(8, 4, 4), (5, 3, 3)])
@pytest.mark.parametrize("K", [1, 2, 5])
def test_sliced_accel_equals_independent_accels(backend, K, res):
    """Bit for bit, slice by slice: ``occ_val``, the thresholds and ``occ_bits`` after init, after two refresh steps and after a
    collect equal K ``DensityOccGridAccel``s fed each slice's points.  Slice 1 (K = 5) never receives a point: it only decays."""
    from neuralsim_amd.fields.dynamic_nerf import DynamicDensityOccGridAccel
    from neuralsim_amd.fields.nerf import DensityOccGridAccel
    kw = dict(resolution=list(res), occ_thre=0.05, ema_decay=0.9, occ_thre_consider_mean=True, constant_value=0.02,
              update_from_samples_cfg={})
    dyn = DynamicDensityOccGridAccel(AABB, keyframes(K), device=backend, **kw)
    ind = [DensityOccGridAccel(AABB, device=backend, **kw) for _ in range(K)]
    nvox, nw = res[0] * res[1] * res[2], (res[0] * res[1] * res[2] + 31) // 32
    assert dyn.occ_val.shape == (K * nvox,) and dyn.occ_bits.shape == (K * nw,) and dyn.occ_grid.shape == (K, *res)

    def same(what, bits=True):
        for k in range(K):
            assert torch.equal(dyn.occ_val[k * nvox:(k + 1) * nvox], ind[k].occ_val), (what, k)
            if bits:
                assert torch.equal(dyn.occ_bits[k * nw:(k + 1) * nw], ind[k].occ_bits), (what, k)
            assert torch.equal(dyn.occ_thre_dev[k:k + 1], ind[k].occ_thre_dev.reshape(1)), (what, k)
            assert torch.equal(dyn.occ_grid[k], ind[k].occ_grid), (what, k)
        if nvox & 31:          # padding bits of every slice's last word are never set
            last = dyn.occ_bits.view(K, nw)[:, -1].cpu()
            assert bool(((last >> (nvox & 31)) == 0).all()), what
    dyn.init()
    for a in ind:
        a.init()
    assert dyn.frac_occupied() == 1.0
    same("init", bits=False)        # (a single grid's init sets the padding bits of its last word as well: compared as occ_grid)
    g = torch.Generator().manual_seed(5 + K)
    for step in range(2):
        n = 300
        pts = (AABB[0] + torch.rand(n, 3, generator=g) * (AABB[1] - AABB[0]) * 1.1 - 0.05).to(backend)      # a few outside
        sig = (torch.rand(n, generator=g) ** 4 * 0.3).to(backend)
        sl = torch.randint(0, K, (n,), generator=g)
        if K == 5:
            sl[sl == 1] = 3
        sl = sl.to(backend)
        before = dyn.occ_val.clone()
        dyn.update_from_samples(pts, sig, sl)
        for k in range(K):
            sel = sl == k
            ind[k].update_from_samples(pts[sel].contiguous(), sig[sel].contiguous())
        same(f"refresh {step}")
        if K == 5:          # the slice without a point only decayed
            assert torch.equal(dyn.occ_val[nvox:2 * nvox], before[nvox:2 * nvox] * 0.9)
    # a point never touches another slice: everything into the last slice
    before = dyn.occ_val.clone()
    pts = (AABB[0] + torch.rand(64, 3, generator=g) * (AABB[1] - AABB[0])).to(backend)
    big = torch.full([64], 7.0, device=backend)
    dyn.collect(big, torch.full([64], K - 1, dtype=torch.long, device=backend), pts=pts)
    ind[K - 1].collect(pts=pts, sigma=big)
    assert torch.equal(dyn.occ_val[:(K - 1) * nvox], before[:(K - 1) * nvox]) and float(dyn.occ_val[(K - 1) * nvox:].max()) == 7.0
    # collect through rays: per-ray slices, no decay, bits untouched until pack_bits
    R = 6
    o = torch.tensor([-3.0, 0.1, -0.2]).repeat(R, 1).to(backend)
    d = torch.tensor([1.0, 0.05, 0.02]).repeat(R, 1).to(backend)
    ridx = torch.arange(R).repeat_interleave(7).to(backend)
    t = (1.2 + 0.5 * torch.arange(7, dtype=torch.float32)).repeat(R).to(backend)
    sg = (torch.rand(R * 7, generator=g) * 3).to(backend)
    rsl = (torch.arange(R) % K).to(backend)
    bits_before = dyn.occ_bits.clone()
    dyn.collect(sg, rsl, rays=(o, d, t, ridx))
    assert torch.equal(dyn.occ_bits, bits_before)
    for k in range(K):
        sel = (rsl[ridx] == k).nonzero()[:, 0]
        if sel.numel():
            x = o[ridx[sel]] + t[sel, None] * d[ridx[sel]]
            ind[k].collect(pts=x.contiguous(), sigma=sg[sel].contiguous())
    dyn.pack_bits()
    for a in ind:
        a.pack_bits()
    same("collect")


# ------------------------------------------------------------------------------------------------ 5. marching
@pytest.mark.parametrize("R", [1, 5, 70])
def test_marching_per_slice(backend, R):
    """Counts and t of the model's query equal the existing marcher run once per slice on that slice's words, with
    ``ray_word_off = NULL``, over that slice's rays."""
    from neuralsim_amd import _lib
    from neuralsim_amd.graphics import pack_ops as po
    m, p, occ = build(backend, 1, 4, 0, "f32")
    if R == 70:         # the rays of the last slice march nothing
        occ[-1] = False
        m.accel.occ_val[-m.accel.nvox:].zero_()
        m.accel.pack_bits()
    tested, ret = run_query(m, backend, R, with_rgb=False)
    r = rays(R)
    assert torch.equal(tested["rays_inds"].cpu(), r["hit"].nonzero()[:, 0]) and torch.equal(tested["rays_ts"].cpu(), r["ts"][r["hit"]])
    Rh = int(tested["num_rays"])
    if Rh == 0:
        assert ret["volume_buffer"]["type"] == "empty"
        return
    acc = m.accel
    sl = acc.slice_of(tested["rays_ts"])
    counts = ret["details"]["march_counts"].cpu()
    t_all = ret["volume_buffer"]["t"].cpu() if ret["volume_buffer"]["type"] != "empty" else torch.zeros(0)
    start = torch.cumsum(counts, 0) - counts
    seen = 0
    for k in range(acc.K):
        sel = (sl == k).nonzero()[:, 0]
        if sel.numel() == 0:
            continue
        o, d = tested["rays_o"][sel].contiguous(), tested["rays_d"][sel].contiguous()
        near, far = tested["near"][sel].contiguous(), tested["far"][sel].contiguous()
        jit = torch.zeros(sel.numel(), device=backend)
        bits = acc.occ_bits[k * acc.words_per_slice:(k + 1) * acc.words_per_slice].contiguous()
        cnt = torch.empty([sel.numel()], dtype=torch.long, device=backend)
        _lib.call("nsim_march_count", _lib.ptr(o), _lib.ptr(d), _lib.ptr(near), _lib.ptr(far), _lib.ptr(jit), sel.numel(),
                  _lib.ptr(bits), None, acc.meta, STEP, MAX_STEPS, _lib.ptr(cnt))
        assert torch.equal(cnt.cpu(), counts[sel.cpu()]), k
        pi, tot = po.get_pack_infos_from_n(cnt, return_total=True)
        if int(tot) == 0:
            continue
        tk = torch.empty([int(tot)], dtype=torch.float32, device=backend)
        _lib.call("nsim_march_emit", _lib.ptr(o), _lib.ptr(d), _lib.ptr(near), _lib.ptr(far), _lib.ptr(jit), sel.numel(),
                  _lib.ptr(bits), None, acc.meta, STEP, MAX_STEPS, _lib.ptr(pi), _lib.ptr(tk))
        tk, pi = tk.cpu(), pi.cpu()
        for i, ray in enumerate(sel.cpu().tolist()):
            assert torch.equal(tk[pi[i, 0]:pi[i, 0] + pi[i, 1]], t_all[start[ray]:start[ray] + counts[ray]])
            seen += int(pi[i, 1])
    assert seen == int(counts.sum())
    if R == 70:
        assert int((counts == 0).sum()) > 0 and int(counts.sum()) > 64         # rays that march nothing; more than one block
    (t_ref, _, c_ref, _), _ = ref_march(m, r, occ, (8, 4, 4))
    assert torch.equal(counts, c_ref) and torch.allclose(t_all, t_ref, atol=1e-6)


def test_same_ray_two_times_after_emptying_a_slice(backend):
    m, _, _ = build(backend, 1, 4, 0, "f32")
    o = torch.tensor([[-3.0, 0.1, 0.05]]).repeat(2, 1).to(backend)
    d = torch.tensor([[1.0, 0.02, -0.01]]).repeat(2, 1).to(backend)
    ts = torch.tensor([0.0, 1.0]).to(backend)                   # slices 0 and 2 of (0, 0.5, 1.0)
    acc = m.accel
    acc.set_all_occupied()
    tested = m.ray_test(o, d, near=0.01, rays_ts=ts)
    a = m.ray_query(ray_tested=tested, config=dict(with_rgb=False), return_details=True)
    c = a["details"]["march_counts"].cpu()
    assert int(c[0]) == int(c[1]) > 0
    acc.occ_val[2 * acc.nvox:].zero_()
    acc.pack_bits()
    b = m.ray_query(ray_tested=tested, config=dict(with_rgb=False), return_details=True)
    cb = b["details"]["march_counts"].cpu()
    assert int(cb[0]) == int(c[0]) and int(cb[1]) == 0
    assert torch.equal(b["volume_buffer"]["rays_inds_hit"].cpu(), torch.tensor([0]))
    assert acc.frac_occupied(per_slice=True).cpu().tolist() == [1.0, 1.0, 0.0]


# ------------------------------------------------------------------------------------------------ 6. model query
@pytest.mark.parametrize("R,res", [(1, (8, 4, 4)), (5, (8, 4, 4)), (70, (8, 4, 4)), (5, (5, 3, 3)), (70, (5, 3, 3))])
def test_model_query(backend, R, res):
    """The volume buffer and the per-object images against the restatement: ``perturb`` off, then a given ``_jitter``."""
    m, p, occ = build(backend, 6, 10, 4, "f32", res=res)
    r = rays(R)
    hit = r["hit"]
    Rh = int(hit.sum())
    g = torch.Generator().manual_seed(8)
    for jitter in (None, torch.rand(Rh, generator=g)):
        dv = lambda t: t.to(backend).contiguous()      # noqa: E731
        tested = m.ray_test(dv(r["o"]), dv(r["d"]), near=0.01, rays_ts=dv(r["ts"]), rays_h_appear=dv(r["ha"]))
        cfg = dict(with_rgb=True, depth_use_normalized_vw=False)
        cfg.update(dict(perturb=False) if jitter is None else dict(_jitter=dv(jitter)))
        ret = m.ray_query(ray_input=dict(rays_o=dv(r["o"]), rays_d=dv(r["d"])), ray_tested=tested, config=cfg,
                          return_details=True, render_per_obj_individual=True)
        (t, ridx, counts, pi), sl = ref_march(m, r, occ, res, jitter)
        assert torch.equal(ret["details"]["slices"].cpu(), sl)
        if int(counts.sum()) == 0:
            assert ret["volume_buffer"]["type"] == "empty" and ret["rendered"]["mask_volume"].shape == (R,)
            continue
        vb = ret["volume_buffer"]
        assert vb["type"] == "packed" and "nablas" not in vb
        assert torch.equal(ret["details"]["march_counts"].cpu(), counts) and torch.allclose(vb["t"].cpu(), t, atol=1e-6)
        assert torch.equal(ret["details"]["ridx"].cpu(), ridx) and torch.equal(ret["details"]["pack_infos"].cpu(), pi)
        assert torch.equal(vb["rays_inds_hit"].cpu(), hit.nonzero()[:, 0][counts > 0])
        assert torch.equal(vb["pack_infos_hit"].cpu(), pi[counts > 0])
        with torch.no_grad():
            ref = dr.query_at(p, r["o"][hit], r["d"][hit], r["ts"][hit], vb["t"].cpu(), ridx, STEP, r["ha"][hit])
        assert float((vb["sigma"].detach().cpu() - ref["sigma"]).abs().max()) < 2e-5 * (1 + float(ref["sigma"].detach().max()))
        assert float((vb["rgb"].detach().cpu() - ref["rgb"]).abs().max()) < 2e-5
        assert float((vb["opacity_alpha"].detach().cpu() - ref["opacity_alpha"]).abs().max()) < 2e-4
        want = orr.volume_integration(ref["opacity_alpha"].float(), vb["t"].cpu(), ref["rgb"].float(), None, pi, False)
        rend = ret["rendered"]
        rows = hit.nonzero()[:, 0]
        for k in ("mask_volume", "depth_volume", "rgb_volume"):
            full = torch.zeros(R, *want[k].shape[1:])
            full[rows] = want[k]
            assert rend[k].shape == full.shape and float((rend[k].detach().cpu() - full).abs().max()) < 5e-4, k


def test_empty_results_and_errors(backend):
    m, _, _ = build(backend, 1, 4, 4, "f32")
    r = rays(5)
    dv = lambda t: t.to(backend).contiguous()      # noqa: E731
    with pytest.raises(ValueError, match="rays_ts"):
        m.ray_test(dv(r["o"]), dv(r["d"]), near=0.01)
    with pytest.raises(NotImplementedError, match="rays_ts"):
        m.ray_test(dv(r["o"]), dv(r["d"]), near=0.01, rays_ts=leaf(r["ts"], backend))
    far_away = dv(r["o"] + torch.tensor([0.0, 50.0, 0.0]))
    tested = m.ray_test(far_away, dv(r["d"]), near=0.01, rays_ts=dv(r["ts"]))             # R == 0
    assert tested["num_rays"] == 0
    ret = m.ray_query(ray_input=dict(rays_o=far_away, rays_d=dv(r["d"])), ray_tested=tested, config={}, return_details=True,
                      render_per_obj_individual=True)
    assert ret["volume_buffer"]["type"] == "empty" and ret["rendered"]["rgb_volume"].shape == (5, 3) and ret["details"] == {}
    tested = m.ray_test(dv(r["o"]), dv(r["d"]), near=0.01, rays_ts=dv(r["ts"]))
    with pytest.raises(ValueError, match="rays_h_appear"):
        m.ray_query(ray_tested=tested, config={})
    with pytest.raises(NotImplementedError, match="rays_o"):
        m.ray_query(ray_tested=dict(tested, rays_o=leaf(tested["rays_o"])), config=dict(with_rgb=False))
    with pytest.raises(NotImplementedError, match="requires_grad"):
        m.forward_density(leaf(r["o"], backend), dv(r["ts"]))
    with pytest.raises(NotImplementedError, match="ts.requires_grad"):
        m.forward_density(dv(r["o"]), leaf(r["ts"], backend))
    m.accel.occ_val.zero_()                                                               # nothing marched
    m.accel.pack_bits()
    assert m.accel.frac_occupied() == 0.0
    m.accel.collect_armed = True
    ret = m.ray_query(ray_tested=tested, config=dict(with_rgb=False), return_details=True)
    assert ret["volume_buffer"]["type"] == "empty" and int(ret["details"]["march_counts"].sum()) == 0 and not m.accel.collect_armed
    out = m.sample_pts_uniform(33)
    assert out["sigma"].shape == (33,) and out["x"].shape == (33, 3) and out["ts"].shape == (33,) and out["sigma"].requires_grad
    assert bool(torch.isin(out["ts"].cpu(), keyframes(5)).all())
    assert m.query_density(torch.zeros(0, 3, device=backend), torch.zeros(0, device=backend)).shape == (0,)


# ------------------------------------------------------------------------------------------------ 7. level mask
def test_level_mask(backend):
    """``set_active_levels(3)`` of 6: masked levels give zero features and exactly zero table gradient, and their tables are not
    read -- they hold NaN here."""
    m, p, _ = build(backend, 6, 10, 0, "f32")
    m.set_active_levels(3)
    T2 = 2 * 2 ** 10
    with torch.no_grad():
        m.encoding.flattened_params[3 * T2:] = float("nan")
    q = points(33)
    got = decode(m, backend, q, None)
    pz = copy.deepcopy(p)
    pz.n_active = 3
    pz.requires_grad_(True)
    ref = dr.query_points(pz, q["x"], q["ts"][q["ridx"]], q["d"][q["ridx"]], None, STEP)
    ev = value_errors(got, ref)
    assert ev["sigma"] < 2e-5 and ev["rgb"] < 2e-5 and ev["alpha"] < 2e-4, ev
    (got[1].sum() + got[2].sum()).backward()
    (ref["opacity_alpha"].sum() + ref["rgb"].sum()).backward()
    gg = m.encoding.flattened_params.grad.cpu()
    assert float(gg[3 * T2:].abs().max()) == 0.0 and float(pz.grid.grad[3 * T2:].abs().max()) == 0.0
    assert rel_l2(gg[:3 * T2], pz.grid.grad[:3 * T2]) < 3e-4
    assert bool(torch.isfinite(m.den_w.grad).all())
    m.set_active_levels(None)
    assert m.meta.lotd.n_active_levels == 0 and m.encoding.cfg.pmeta.n_active_levels == 0


# ------------------------------------------------------------------------------------------------ 8. config and state
def _golden_params():
    from nr3d_lib.config import load_config
    cfg = load_config(str(GOLDEN))
    blk = cfg["assetbank_cfg"]["Dynamic"]
    blk = blk.to_dict() if hasattr(blk, "to_dict") else dict(blk)
    return blk


def test_yaml_fixture_constructs_through_the_shim():
    """The reference's own ``assetbank_cfg.Dynamic`` block (interpolations resolved) constructs the model through the shim
    class, the way app/models/single/dynamic_nerf.py:93-153 drives it (sizes overridden down)."""
    from nr3d_lib.models.accelerations import accel_types_dynamic, get_accel_class
    from nr3d_lib.models.fields_dynamic.nerf import EmerNeRFModel, EmerNeRFOnlyDynamicModel
    from neuralsim_amd.fields import dynamic_nerf as dn
    assert EmerNeRFOnlyDynamicModel is dn.EmerNeRFOnlyDynamicModel
    with pytest.raises(NotImplementedError, match="EmerNeRFModel"):
        EmerNeRFModel()
    blk = _golden_params()
    mp = copy.deepcopy(blk["model_params"])
    assert mp["n_geometry_feat"] == 64 and mp["accel_cfg"]["vox_size"] == 2.0 and mp["radiance_cfg"]["n_appear_embedding"] == 4
    pac = mp["dynamic_encoding_cfg"]["param"]["permuto_auto_compute_cfg"]
    assert pac["n_levels"] == 16 and pac["log2_hashmap_size"] == 19 and pac["finest_res"] == 10000.0
    pac["log2_hashmap_size"] = 8

    class EmerNerfStreetOnlyDynamic(EmerNeRFOnlyDynamicModel):        # what app/models/single/dynamic_nerf.py:93 derives
        def asset_populate(self, ts_keyframes, aabb, config, device=None):
            if self.accel_cfg is not None:
                accel_cls = get_accel_class(self.accel_cfg["type"])
                if accel_cls in accel_types_dynamic:
                    self.accel_cfg.update(ts_keyframes=ts_keyframes[::int(config.get("accel_n_jump_frames", 2))].contiguous())
            super().populate(aabb=aabb, ts_keyframes=ts_keyframes, device=device)

    m = EmerNerfStreetOnlyDynamic(**mp)
    assert m.use_ts and m.is_ray_query_supported
    ts = torch.arange(7, dtype=torch.float32) * 0.1
    m.asset_populate(ts, torch.tensor([[-9.0, -5, -3], [10.0, 5, 3]]), blk["asset_params"]["populate_cfg"])
    assert m.encoding.cfg.num_levels == 16 and m.n_appear == 4 and m.meta.precision == 0
    assert m.accel.K == 4 and m.accel.resolution == [10, 5, 3] and m.accel.occ_thre_consider_mean      # vox_size 2.0; nvox 150
    assert m.accel.words_per_slice == 5 and m.accel.occ_val.shape == (600,) and m.accel.frac_occupied() == 1.0
    assert m.accel.n_steps_warmup == 256 and m.accel.num_pts == 2 ** 22 and m.ray_query_cfg["query_mode"] == "march_occ"
    assert isinstance(m.accel, accel_types_dynamic)
    assert len(m.training_setup(dict(lr=1e-2, eps=1e-15, betas=[0.9, 0.99])).param_groups) == 3
    assert m.get_weight_reg().shape == (2,)


@ref_glue.needs_reference(ref_glue.readable(REF_YAML), reason="reads the reference's yaml, which only the authoring machine has")
def test_yaml_fixture_matches_the_reference():
    from nr3d_lib.config import load_config
    ref = load_config(str(REF_YAML))["assetbank_cfg"]["Dynamic"]
    ref = ref.to_dict() if hasattr(ref, "to_dict") else dict(ref)
    blk = _golden_params()
    ref["asset_params"].pop("training_cfg", None)
    assert blk["model_class"] == ref["model_class"] and blk["model_params"] == ref["model_params"]
    assert blk["asset_params"] == ref["asset_params"]


def test_refused_options_and_state_dict(backend):
    from neuralsim_amd.fields.dynamic_nerf import EmerNeRFOnlyDynamicModel
    enc = lambda **kw: dict(type="permuto", param=dict(permuto_auto_compute_cfg=dict(     # noqa: E731
        dict(type="multi_res", n_levels=6, n_feats=2, log2_hashmap_size=8), **kw)))
    bad = [("use_flow_field", True, "use_flow_field"), ("use_shadow", True, "use_shadow"), ("n_semantic_feat", 8, "n_semantic_feat"),
           ("ray_query_cfg", dict(query_mode="march_occ_multi_upsample"), "query_mode"),
           ("dynamic_encoding_cfg", dict(type="lotd"), "dynamic_encoding_cfg.type"),
           ("dynamic_encoding_cfg", enc(n_feats=4), "n_feats"), ("dynamic_encoding_cfg", enc(n_levels=17), "n_levels"),
           ("time_embedding_cfg", dict(dim=2, learnable=False), "time_embedding_cfg.dim"),
           ("time_embedding_cfg", dict(dim=1, learnable=True), "time_embedding_cfg.learnable"),
           ("static_encoding_cfg", dict(type="permuto"), "EmerNeRFModel"),
           ("n_geometry_feat", 32, "n_geometry_feat"), ("density_activation", "trunc_exp", "density_activation"),
           ("dynamic_decoder_cfg", dict(type="mlp", D=2, W=64), "dynamic_decoder_cfg.D"),
           ("radiance_cfg", dict(use_nablas=True, D=2, W=64), "use_nablas"),
           ("accel_cfg", dict(type="occ_grid"), "accel_cfg.type")]
    for key, val, word in bad:
        with pytest.raises(NotImplementedError, match=word):
            EmerNeRFOnlyDynamicModel(**yaml_params(**{key: val}))
    assert EmerNeRFOnlyDynamicModel(**yaml_params(density_activation="trunc_softplus")).cfgd["n_appear"] == 0
    m, _, _ = build(backend, 6, 10, 4, "f32")
    m.accel.occ_val.mul_(torch.rand(m.accel.occ_val.shape, generator=torch.Generator().manual_seed(1)).to(backend) + 0.5)
    fresh = EmerNeRFOnlyDynamicModel(**yaml_params(6, 10, 4))
    fresh.populate(aabb=AABB, ts_keyframes=keyframes(5) + 1.0, accel_n_jump_frames=2, device=backend)
    sd = m.state_dict()
    assert "accel.occ_val" in sd and "ts_keyframes" in sd and "accel.ts_keyframes" in sd
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.ts_keyframes, m.ts_keyframes) and torch.equal(fresh.accel.occ_val, m.accel.occ_val)
    assert torch.equal(fresh.accel.occ_bits, m.accel.occ_bits)
    ha = rays(5)["ha"].to(backend)
    with torch.no_grad():
        _, a = run_query(m, backend, 5, ha, with_rgb=True)
        _, b = run_query(fresh, backend, 5, ha, with_rgb=True)
    for k in ("t", "sigma", "opacity_alpha", "rgb", "pack_infos_hit", "rays_inds_hit"):
        assert torch.equal(a["volume_buffer"][k], b["volume_buffer"][k]), k


# ------------------------------------------------------------------------------------------------ 9. compose
def test_compose_with_street_neus(backend):
    """A street NeuS drawable plus a ``Dynamic`` drawable through ``BufferComposeRenderer`` with ``rays_ts``: the joint buffer
    equals the reference's collect / sort / integrate steps (oracle/render.py compose_buffers) applied to the two models' own
    buffers; without the ``Dynamic`` drawable and without ``rays_ts`` the call returns what it returned before."""
    from neuralsim_amd.fields.neus import OccGridAccel
    from neuralsim_amd.renderers.buffer_compose_renderer import BufferComposeRenderer, Drawable
    from util import make_params, model_from_params
    box = torch.tensor([[-1.0, -1, -1], [1.0, 1, 1]])
    pm = make_params(sdf_D=2, small=True, sphere=True, seed=11, ln_inv_s=0.45, grid_bound=2e-2, noise_scale=1.0)
    main = model_from_params(pm, backend, precision="f32")
    main.accel = OccGridAccel(box, resolution=[8, 8, 8], device=backend)
    main.accel.set_all_occupied()
    main.ray_query_cfg = dict(query_mode="march_occ_multi_upsample",
                              query_param=dict(num_coarse=8, num_fine=[4, 4], upsample_inv_s=64.0, upsample_inv_s_factors=[1, 4],
                                               march_cfg=dict(step_size=0.05, max_steps=128)))
    dyn, _, _ = build(backend, 6, 10, 4, "f32")
    R = 70
    r = rays(R)
    dv = lambda a: a.to(backend).contiguous()      # noqa: E731
    o = r["o"] * torch.tensor([0.6, 1.0, 1.0])      # closer: most rays cross both boxes
    rend = BufferComposeRenderer(dict(with_rgb=True, with_normal=False, near=0.01, depth_use_normalized_vw=True)).train()
    byp = dict(Street=dict(perturb=False), Dynamic=dict(perturb=False))
    both = [Drawable("street", "Street", main), Drawable("dyn", "Dynamic", dyn)]
    with torch.no_grad():
        ret = rend(dv(o), dv(r["d"]), drawables=both, rays_h_appear=dv(r["ha"]), rays_ts=dv(r["ts"]), return_buffer=True,
                   return_details=True, bypass_ray_query_cfg=byp)
        alone_ts = rend(dv(o), dv(r["d"]), drawables=both[:1], rays_h_appear=dv(r["ha"]), rays_ts=dv(r["ts"]), return_buffer=True,
                        bypass_ray_query_cfg=byp)
        alone = rend(dv(o), dv(r["d"]), drawables=both[:1], rays_h_appear=dv(r["ha"]), return_buffer=True, bypass_ray_query_cfg=byp)
    raws = ret["raw_per_obj_model"]
    assert set(raws) == {"street", "dyn"} and all(v["volume_buffer"]["type"] == "packed" for v in raws.values())
    bufs = [dict(rays_inds=v["volume_buffer"]["rays_inds_hit"].cpu(), pack_infos=v["volume_buffer"]["pack_infos_hit"].cpu(),
                 t=v["volume_buffer"]["t"].cpu(), alpha=v["volume_buffer"]["opacity_alpha"].cpu(), rgb=v["volume_buffer"]["rgb"].cpu())
            for v in raws.values()]
    mask_o, depth_o, rgb_o, cnt_o = orr.compose_buffers(bufs, R, True)
    assert torch.equal(ret["ray_intersections"]["samples_cnt"].cpu(), cnt_o)
    assert int((cnt_o > int(bufs[0]["pack_infos"][:, 1].max())).sum()) > 0          # rays that carry samples of both models
    rr = ret["rendered"]
    # (bounds of tests/test_compose.py)
    assert (rr["mask_volume"].cpu() - mask_o).abs().max() < 5e-4 and (rr["rgb_volume"].cpu() - rgb_o).abs().max() < 5e-4
    assert (rr["depth_volume"].cpu() - depth_o).abs().max() < 2e-3
    tvb = ret["volume_buffer"]
    assert int(tvb["pack_infos_hit"][:, 1].sum()) == int(cnt_o.sum())
    for k in ("mask_volume", "depth_volume", "rgb_volume"):
        assert torch.equal(alone["rendered"][k], alone_ts["rendered"][k]), k
    for k in ("t", "opacity_alpha", "rgb", "pack_infos_hit", "rays_inds_hit"):
        assert torch.equal(alone["volume_buffer"][k], alone_ts["volume_buffer"][k]), k
    with pytest.raises(ValueError, match="rays_ts"):
        rend(dv(o), dv(r["d"]), drawables=both, rays_h_appear=dv(r["ha"]))


# ------------------------------------------------------------------------------------------------ 10. training steps
def test_dynamic_nerf_training_steps(backend):
    """30 Adam steps (the package's optimizer) on one fixed batch whose target is rendered from a second model of another seed at
    three ray times, driven through ``training_before_per_step`` (the refresh on a shortened schedule, the sample collection):
    the loss ends below its start, parameters stay finite; every slice is fully occupied before the first refresh and at least
    one is not after it."""
    from neuralsim_amd.fields.neus import volume_integration
    R = 21
    g = torch.Generator().manual_seed(4)
    base = rays(70)
    rows = base["hit"].nonzero()[:R, 0]
    o, d = base["o"][rows], base["d"][rows]
    ts = torch.tensor([0.0, 0.5, 1.0])[torch.arange(R) % 3]
    dv = lambda t: t.to(backend).contiguous()      # noqa: E731
    scene, _, _ = build(backend, 6, 10, 0, "f32", seed=23)
    m, _, _ = build(backend, 6, 10, 0, "f32", seed=11)
    scene.accel.set_all_occupied()
    with torch.no_grad():
        tested_s = scene.ray_test(dv(o), dv(d), near=0.01, rays_ts=dv(ts))
        gt = scene.ray_query(ray_input=dict(rays_o=dv(o), rays_d=dv(d)), ray_tested=tested_s,
                             config=dict(with_rgb=True, perturb=False, depth_use_normalized_vw=False),
                             render_per_obj_individual=True)["rendered"]["rgb_volume"]
    assert gt.shape == (R, 3) and float(gt.abs().sum()) > 0
    tested = m.ray_test(dv(o), dv(d), near=0.01, rays_ts=dv(ts))
    opt = m.training_setup(dict(lr=1e-2, eps=1e-15, betas=[0.9, 0.99]))
    m.training_initialize()
    assert m.accel.frac_occupied(per_slice=True).cpu().tolist() == [1.0] * m.accel.K
    m.accel.n_steps_warmup, m.accel.n_steps_between_update = 8, 8      # the refresh runs at it = 8, 16, 24
    m.refresh_generator = torch.Generator(device=backend).manual_seed(3)
    losses, fracs = [], []
    for it in range(30):
        m.training_before_per_step(it)
        assert m.accel.collect_armed
        fracs.append(m.accel.frac_occupied(per_slice=True).cpu())
        gen = torch.Generator(device=backend).manual_seed(0)      # rewound point stream, jitter 0: a fixed objective
        ret = m.ray_query(ray_tested=tested, config=dict(with_rgb=True, _jitter=torch.zeros(tested["num_rays"], device=backend)),
                          return_details=True)
        assert not m.accel.collect_armed
        vb = ret["volume_buffer"]
        rend = volume_integration(vb["opacity_alpha"], vb["t"], vb["rgb"], None, ret["details"]["pack_infos"], False,
                                  rays_inds=tested["rays_inds"], num_rays=R)
        loss = ((rend["rgb_volume"] - gt) ** 2).mean() + 1e-3 * m.sample_pts_uniform(64, generator=gen)["sigma"].mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        m.training_after_per_step(it)
        losses.append(float(loss.detach()))
    assert bool((fracs[7] == 1.0).all()) and bool((fracs[8] < 1.0).any()) and float(m.accel.occ_val.max()) > 1.0e-2
    assert losses[-1] < losses[0], losses
    assert all(bool(torch.isfinite(q_).all()) for q_ in m.parameters())
