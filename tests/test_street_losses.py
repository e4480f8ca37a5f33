"""The street configs' supervision losses (app/loss/{mask, mask_entropy, sparsity, clearance, lidar}.py):
``neuralsim_amd.losses.{mask_occupancy_loss, object_mask_in_total, mask_entropy_loss, sparsity_loss, clearance_loss, kth_value,
lidar_loss}``, their C-ABI launch budget, the replay of the reference's own classes from tests/golden/street_loss_fixture.pt, and
``RenderTrainer(loss_cfg=)`` -- against the float64 restatement tests/street_loss_ref.py.

Bounds.  Every case evaluates the restatement twice on the CPU, in float64 (the reference value) and in float32 torch ops.  The
kernels are allowed 8 x that float32 run's departure from float64 -- in the value, |v - v64|, and in the gradient, max |g - g64| /
max |g64| -- with a floor of 1e-6 relative; no element is exempt.  The margin covers another summation order and the float
atomics of the reductions.  Against the frozen float32 run of the reference's classes the allowance is doubled (both runs lie
within one bound of float64).  Discrete decisions -- ``kth_value``, the validity and outlier masks, the line-of-sight membership,
which side of a clamp passes the gradient -- are compared exactly; the random inputs keep every error 1e-3 (relative) away from
median x factor and every |t - gt| 1e-4 away from epsilon / sigma (asserted on the inputs first), and separate cases put
exactly representable values ON the thresholds.

Measured departures of the float32 CPU run from float64 over the cases of this file, and the kernels' own on the emulator
(the largest of each over the cases, the value relative to |v64|, the gradient to max |g64|):

    op                 f32 torch value   f32 torch grad    kernel value   kernel grad
    mask BCE           1.9e-7            1.5e-7            1.2e-7         1.4e-7
    mask entropy       1.9e-7            6.4e-7            1.1e-7         8.0e-7
    sparsity           1.0e-6            8.9e-7            1.0e-6         8.9e-7
    clearance          5.2e-8            1.2e-7            5.2e-8         9.7e-8
    lidar (3 sums)     9.5e-6            6.4e-6            2.3e-7         1.3e-7

The sparsity figure is a rounding both runs share (lamb = 0.05 is no float32).  The torch run's lidar figures are ``log(pred + 1) -
log(gt + 1)`` and ``pred / far - gt / far``: differences of nearly equal rounded numbers.  The kernel takes both between the inputs
(``log1p((pred - gt) / (gt + 1))``, ``(pred - gt) / far``) and stays at 2e-7 -- with the difference of two ``logf`` it sat AT the torch
run's error, and on the device (another ``logf``) one value of the replay crossed its bound by 0.05 %.  In most cases the floor of
1e-6 is the bound that binds."""
import math
from pathlib import Path

import pytest
import torch

import street_loss_ref as ref
from conftest import sync
from neuralsim_amd import _lib, losses
from util import leaf

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = ROOT / "tests" / "golden" / "street_loss_fixture.pt"
NS = [1, 63, 64, 65, 300]
FLOOR, MARGIN = 1e-6, 8.0
COEF = (1.0, 0.7, 1.3)          # upstream gradients of the (up to three) sums of one call: each its own


def _check(tag, vals, grads, r32, r64, mult=1.0, target=None):
    """vals: dict key -> 0-dim tensor; grads: list of tensors; r32 / r64: (dict of values, list of gradients) of the restatement,
    which set the bound; ``target`` (default: r64): what the values and gradients are compared with"""
    target = r64 if target is None else target
    assert set(vals) == set(r64[0]), (tag, sorted(vals), sorted(r64[0]))
    for k, v in vals.items():
        v64, v32, vt = float(r64[0][k]), float(r32[0][k]), float(target[0][k])
        assert v.shape == () and v.dtype == torch.float32
        got = float(v.detach())
        tol = mult * max(MARGIN * abs(v32 - v64), FLOOR * abs(v64))
        print(f"{tag} {k}: value {got:.7e} err {abs(got - vt):.2e} (f32 torch {abs(v32 - v64):.2e}, bound {tol:.2e})")
        assert math.isfinite(got) and abs(got - vt) <= tol, (tag, k, got, vt, tol)
    assert len(grads) == len(r64[1])
    for j, (g, g32, g64) in enumerate(zip(grads, r32[1], r64[1])):
        assert g is not None and g.shape == g64.shape and bool(torch.isfinite(g).all()), (tag, j)
        scale = float(g64.abs().max())
        e = float((g.detach().cpu().double() - target[1][j]).abs().max())
        if scale == 0.0:
            print(f"{tag} grad {j}: zero gradient, max |g| {e:.2e}")
            assert e == 0.0, (tag, j, e)
            continue
        e32 = float((g32.double() - g64).abs().max())
        tol = mult * max(MARGIN * e32 / scale, FLOOR)
        print(f"{tag} grad {j}: err {e / scale:.2e} max|g64| (f32 torch {e32 / scale:.2e}, bound {tol:.2e})")
        assert e / scale <= tol, (tag, j, e / scale, tol)


def _ref_run(fn, inputs):
    """fn(dtype, *leaves) -> dict of losses; -> ((values, grads) in float32, (values, grads) in float64)"""
    out = []
    for dtype in (torch.float32, torch.float64):
        ls = [leaf(x, dtype=dtype) for x in inputs]
        vals = fn(dtype, *ls)
        tot = sum(c * v for c, v in zip(COEF, vals.values()))
        if torch.is_tensor(tot) and tot.requires_grad:
            tot.backward()
        out.append(({k: v.detach() for k, v in vals.items()}, [x.grad if x.grad is not None else torch.zeros_like(x) for x in ls]))
    return out


def _op_run(fn, inputs, backend):
    ls = [leaf(x, backend) for x in inputs]
    vals = fn(*ls)
    tot = sum(c * v for c, v in zip(COEF, vals.values()))
    if torch.is_tensor(tot) and tot.requires_grad:
        tot.backward()
    sync(backend)
    return vals, [x.grad if x.grad is not None else torch.zeros_like(x) for x in ls]


# ------------------------------------------------------------------------------------------------ 1. occupancy mask
MASK_CFGS = [dict(safe_bce=True, pred_clip=0),                    # the yaml (withmask_withlidar_joint.240219.yaml:438-441)
             dict(),                                             # the constructor's defaults: clip 1e-3, then the safe clamp
             dict(safe_bce=True, pred_clip=0.2, bce_limit=0.1),   # the clip is the tighter one
             dict(safe_bce=False, pred_clip=1.0e-3),
             dict(safe_bce=False, pred_clip=0.0)]                # no clamp at all: the -100 floor of the logs is reached


def _mask_inputs(N, cfg, seed):
    g = torch.Generator().manual_seed(seed)
    lo, hi = ref.mask_clamp(cfg.get("pred_clip", 1.0e-3), cfg.get("safe_bce", True), cfg.get("bce_limit", 0.1))
    special = torch.tensor([lo, hi, 0.0, 1.0, 0.5 * lo, hi + 0.5 * (1.0 - hi), 0.5], dtype=torch.float32)     # on, outside, inside
    pred = torch.cat([special, torch.rand(max(N, 7), generator=g) * 1.1 - 0.05])[:N].clamp(0.0, 1.0)
    if N > 7:
        pred[7] = -0.01                       # a rendering may overshoot by rounding; outside [0, 1] on both sides
    if N > 8:
        pred[8] = 1.01
    gt = torch.cat([torch.tensor([1.0, 0.0, 0.0, 1.0, 0.3, 0.75, 0.5]), (torch.rand(max(N, 7), generator=g) > 0.5).float()])[:N]
    return pred, gt


@pytest.mark.parametrize("mode", [None, "always_occupied", "only_cull_non_occupied", "only_preserve_occupied"])
@pytest.mark.parametrize("N", NS)
def test_mask_occupancy_matches_float64(backend, N, mode):
    for ci, cfg in enumerate(MASK_CFGS):
        if cfg.get("safe_bce", True) is False and cfg["pred_clip"] == 0.0 and N > 8:
            continue                          # (pred outside [0, 1] without a clamp is a NaN in every implementation)
        pred, gt = _mask_inputs(N, cfg, 100 + N)
        kw = dict(cfg, special_mask_mode=mode, w=0.3)
        r32, r64 = _ref_run(lambda dt, p: {"loss_mask": ref.mask_occupancy(p, gt, dt, **kw)[0]}, [pred])
        err_holder = {}

        def run(p):
            loss, err = losses.mask_occupancy_loss(p, None if mode == "always_occupied" else gt.to(backend), **kw)
            err_holder["err"] = err
            return {"loss_mask": loss}
        vals, grads = _op_run(run, [pred], backend)
        _check(f"mask N={N} mode={mode} cfg{ci}", vals, grads, r32, r64)
        err = err_holder["err"]
        assert not err.requires_grad and err.shape == pred.shape
        assert torch.equal(err.cpu(), ref.mask_occupancy(pred, gt, torch.float32, **kw)[1])          # one subtraction: exact
        lo, hi = ref.mask_clamp(cfg.get("pred_clip", 1.0e-3), cfg.get("safe_bce", True), cfg.get("bce_limit", 0.1))
        outside = (pred < lo) | (pred > hi)
        assert torch.equal(grads[0].cpu()[outside], torch.zeros(int(outside.sum())))                # the clamp's dead zone, exactly
        if mode is None and N >= 2 and lo > 0:
            assert float(grads[0].cpu()[0]) != 0.0 and float(grads[0].cpu()[1]) != 0.0              # ON the bounds: passed


def test_mask_occupancy_refusals(backend):
    p, g = torch.rand(8, device=backend), torch.rand(8, device=backend)
    with pytest.raises(NotImplementedError, match="special_mask_mode"):
        losses.mask_occupancy_loss(p, g, special_mask_mode="never")
    with pytest.raises(TypeError):
        losses.mask_occupancy_loss(p, g, limit=0.1)
    with pytest.raises(NotImplementedError, match="gt.requires_grad"):
        losses.mask_occupancy_loss(p, g.clone().requires_grad_(True))
    loss, err = losses.mask_occupancy_loss(p.view(2, 4).t(), g.view(2, 4).t())                      # non-contiguous inputs
    l2, _ = losses.mask_occupancy_loss(p.view(2, 4).t().contiguous(), g.view(2, 4).t().contiguous())
    assert err.shape == (4, 2) and float(loss) == float(l2)


# ------------------------------------------------------------------------------------------------ 2. mask entropy
def _packed_object(N, seed, absent_every=4):
    """a close-range object's buffer in the total rendering: packs of 1 sample, one of 200, rays it does not touch"""
    g = torch.Generator().manual_seed(seed)
    hit = torch.tensor([i for i in range(N) if N < 3 or i % absent_every != 1], dtype=torch.long)
    n = torch.randint(2, 13, [hit.shape[0]], generator=g)
    n[::3] = 1
    if hit.shape[0] > 1:
        n[1] = 200
    pi = torch.stack([torch.cumsum(n, 0) - n, n], dim=1)
    S = int(n.sum())
    seg = torch.repeat_interleave(torch.arange(hit.shape[0]), n)
    vw = torch.rand(S, generator=g)
    share = torch.rand(hit.shape[0], generator=g)
    share[::5] = 0.0                                                                                # an object that is there, unseen
    vw = vw / torch.zeros(hit.shape[0]).index_add(0, seg, vw)[seg] * share[seg]
    return dict(type="packed", rays_inds_collect=hit, pack_infos_collect=pi, vw_in_total=vw)


def _distant_object(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    vw = torch.rand(N * K, generator=g) / K * 0.9
    n = torch.full([N], K, dtype=torch.long)
    return dict(type="packed", rays_inds_collect=torch.arange(N), pack_infos_collect=torch.stack([torch.cumsum(n, 0) - n, n], 1),
                vw_in_total=vw)


def _to(vb, dev, **repl):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in dict(vb, **repl).items()}


@pytest.mark.parametrize("mode", ref.ENTROPY_MODES)
def test_mask_entropy_every_mode_matches_float64(backend, mode):
    """masks handed in directly, with 0, 1, eps and 1 - eps among them (eps as the float32 the kernels compare with)"""
    N, eps = 300, 1.0e-5
    e32 = ref.f32(eps)
    g = torch.Generator().manual_seed(7)
    special = torch.tensor([0.0, 1.0, e32, 1.0 - e32, 0.5 * e32, 0.25], dtype=torch.float32)
    masks = [torch.cat([special.roll(s), torch.rand(N - 6, generator=g)]) for s in (0, 2, 4)]
    kw = dict(eps=eps, w=0.005)
    r32, r64 = _ref_run(lambda dt, p, cr, dv: ref.mask_entropy(mode, dt, mask_pred=p, mask_cr=cr, mask_dv=dv, eps=e32, w=0.005), masks)
    vals, grads = _op_run(lambda p, cr, dv: losses.mask_entropy_loss(mode, mask_pred=p, mask_cr=cr, mask_dv=dv, **kw), masks, backend)
    _check(f"entropy {mode}", vals, grads, r32, r64)          # (a detached mask: a gradient of exact zeros, checked as such)
    if mode == "nop":
        assert vals == {}


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("mode,cr_empty", [("crisp_cr", False), ("cross_crdv", False), ("crisp_cr", True), ("cross_cr_on_dv", True)])
def test_mask_entropy_on_object_buffers(backend, N, mode, cr_empty):
    """the masks built from the objects' buffers (``object_mask_in_total``), gradients down to ``vw_in_total``"""
    cr = dict(type="empty") if cr_empty else _packed_object(N, 20 + N)
    dv = _distant_object(N, 5, 30 + N)
    leaves = [dv["vw_in_total"]] + ([] if cr_empty else [cr["vw_in_total"]])

    def fn_ref(dt, vdv, vcr=None):
        m_cr = ref.object_mask_in_total(cr if cr_empty else dict(cr, vw_in_total=vcr), N, dt)
        return ref.mask_entropy(mode, dt, mask_cr=m_cr, mask_dv=ref.object_mask_in_total(dict(dv, vw_in_total=vdv), N, dt),
                                eps=ref.f32(1e-5), w=0.25)

    def fn_op(vdv, vcr=None):
        m_cr = losses.object_mask_in_total(cr if cr_empty else _to(cr, backend, vw_in_total=vcr), N, device=backend)
        m_dv = losses.object_mask_in_total(_to(dv, backend, vw_in_total=vdv), N)
        if cr_empty:
            assert torch.equal(m_cr.cpu(), torch.zeros(N))
        return losses.mask_entropy_loss(mode, mask_cr=m_cr, mask_dv=m_dv, w=0.25)
    r32, r64 = _ref_run(fn_ref, leaves)
    vals, grads = _op_run(fn_op, leaves, backend)
    _check(f"entropy buffers N={N} {mode} empty={cr_empty}", vals, grads, r32, r64)


def test_mask_entropy_refusals(backend):
    m = torch.rand(8, device=backend)
    with pytest.raises(NotImplementedError, match="mode"):
        losses.mask_entropy_loss("crisp_sky", mask_pred=m)
    with pytest.raises(ValueError, match="mask_dv"):
        losses.mask_entropy_loss("cross_cr_on_dv", mask_cr=m)
    with pytest.raises(TypeError):
        losses.mask_entropy_loss("crisp", mask_pred=m, anneal=None)
    assert losses.mask_entropy_loss("nop") == {}
    assert set(losses.MASK_ENTROPY_MODES) == set(ref.ENTROPY_MODES)


# ------------------------------------------------------------------------------------------------ 3. sparsity / clearance
@pytest.mark.parametrize("M", [1, 257])
@pytest.mark.parametrize("type_,param", [("normalized_logistic_density", dict(inv_scale=16.0)), ("normalized_logistic_density", {}),
                                         ("normal", dict(std=2.0)), ("normal", {}), ("density_reg", dict(lamb=0.05)),
                                         ("density_reg", dict(lamb=3.0))])
def test_sparsity_matches_float64(backend, M, type_, param):
    g = torch.Generator().manual_seed(40 + M)
    x = torch.randn(M, generator=g) * 0.2
    if type_ == "normal":
        x = x.abs() + 0.01                          # a density: x ** std of a negative x is not what the function is for
    if type_ == "density_reg" and M > 1:
        x[3] = 0.0                                  # |.| at its kink: sub-gradient 0
    r32, r64 = _ref_run(lambda dt, v: {"loss_sparsity": ref.sparsity(v, type_, w=0.02, **param)}, [x])
    vals, grads = _op_run(lambda v: {"loss_sparsity": losses.sparsity_loss(v, type_, w=0.02, **param)}, [x], backend)
    _check(f"sparsity {type_} {param} M={M}", vals, grads, r32, r64)
    if type_ == "density_reg" and M > 1:
        assert float(grads[0].cpu()[3]) == 0.0


@pytest.mark.parametrize("M", [1, 257])
@pytest.mark.parametrize("above", [False, True])
def test_clearance_matches_float64(backend, M, above):
    g = torch.Generator().manual_seed(50 + M)
    thresh, beta = 0.01, 10.0
    x = torch.randn(M, generator=g) * 0.05 if not above else 0.02 + torch.rand(M, generator=g)
    if M > 1 and not above:
        x[0] = ref.f32(thresh)                      # ON the threshold: ``<`` is strict, not penalised
    if M == 1 and not above:
        x[0] = -0.03
    below = x < thresh                              # float32 against the float32 threshold
    assert bool(below.any()) != above
    th = ref.f32(thresh)
    r32, r64 = _ref_run(lambda dt, v: {"loss_clearance": ref.clearance(v, below, beta, th, w=0.1)}, [x])
    vals, grads = _op_run(lambda v: {"loss_clearance": losses.clearance_loss(v, beta=beta, thresh=thresh, w=0.1)}, [x], backend)
    if above:                                       # zero, with zero gradient, and a tensor that is still part of the graph
        assert float(vals["loss_clearance"].detach()) == 0.0 and vals["loss_clearance"].requires_grad
        assert torch.equal(grads[0].cpu(), torch.zeros(M))
        return
    _check(f"clearance M={M}", vals, grads, r32, r64)
    assert torch.equal(grads[0].cpu()[~below], torch.zeros(int((~below).sum())))


def test_point_loss_refusals(backend):
    x = torch.rand(8, device=backend)
    with pytest.raises(NotImplementedError, match="type"):
        losses.sparsity_loss(x, "laplace")
    with pytest.raises(TypeError, match="std"):
        losses.sparsity_loss(x, "normalized_logistic_density", std=1.0)
    with pytest.raises(TypeError):
        losses.clearance_loss(x, gamma=1.0)
    v = losses.sparsity_loss(x.view(2, 4).t())      # non-contiguous, any shape
    assert v.shape == () and abs(float(v) - float(losses.sparsity_loss(x))) <= 1e-6


# ------------------------------------------------------------------------------------------------ 4. exact order statistic
def _kth_inputs(N, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        return torch.randn(N, generator=g).abs() * 10.0
    if kind == "equal":
        return torch.full([N], 0.37)
    if kind == "half_zeros":
        x = torch.rand(N, generator=g)
        x[torch.randperm(N, generator=g)[: (N + 1) // 2]] = 0.0
        return x
    if kind == "last_bit":                      # four neighbouring floats, shuffled
        base = torch.tensor(1.5).view(torch.int32)
        return (base + torch.randint(0, 4, [N], generator=g, dtype=torch.int32)).view(torch.float32)
    if kind == "denormal":                      # bit patterns 0 .. 2^20: zeros, denormals, nothing normal
        return torch.randint(0, 1 << 20, [N], generator=g, dtype=torch.int32).view(torch.float32)
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["random", "equal", "half_zeros", "last_bit", "denormal"])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257, 4099])
def test_kth_value_is_the_sorted_element_bit_for_bit(backend, N, kind):
    x = _kth_inputs(N, kind, 60 + N)
    want = torch.sort(x).values
    xd = x.to(backend)
    for k in sorted({0, N // 2, N - 1}):
        got = losses.kth_value(xd, k)
        sync(backend)
        assert got.shape == () and got.dtype == torch.float32 and got.device.type == backend.type and not got.requires_grad
        assert int(got.cpu().view(torch.int32)) == int(want[k].view(torch.int32)), (N, kind, k, float(got), float(want[k]))
    if N == 65:
        assert int(losses.kth_value(xd.view(5, 13).t(), 32).cpu().view(torch.int32)) == int(want[32].view(torch.int32))
        with pytest.raises(ValueError, match="k"):
            losses.kth_value(xd, N)


# ------------------------------------------------------------------------------------------------ 5. lidar
LIDAR_CFGS = [
    dict(depth=dict(w=0.02, fn_type="l1"), line_of_sight=dict(w=0.1, fn_type="neus_unisim", fn_param=dict(epsilon=1.5))),    # the yaml
    dict(depth=dict(w=0.03, fn_type="l1_log"), line_of_sight=dict(w=0.05, fn_type="nerf", fn_param=dict(sigma=1.5, sigma_scale_factor=3.0))),
    dict(depth=dict(w=0.5, fn_type="l2"), line_of_sight=dict(w=0.2, fn_type="neus_urban", fn_param=dict(sigma=1.0))),
    dict(depth=dict(w=1.0, fn_type="l2_relative")),
    dict(depth=dict(w=1.0, fn_type="l2_normalized"), line_of_sight=dict(fn_type="neus_unisim", fn_param=dict(epsilon=0.5))),
    dict(depth=dict(w=0.1, fn_type="huber", fn_param=dict(alpha=0.3)), line_of_sight=dict(w=0.1)),
    dict(line_of_sight=dict(w=0.1, fn_type="neus_unisim")),
]
TOOFAR, FACTOR = 80.0, 100.0


def _los_bound(cfg):
    los = cfg.get("line_of_sight")
    if los is None:
        return None
    fp = los.get("fn_param") or {}
    return fp.get("epsilon", 1.0) if los.get("fn_type", "nerf") == "neus_unisim" else fp.get("sigma", 1.0)


def _lidar_case(N, seed, bound, invalid_every=7):
    """beams: no return (ranges 0), beyond discard_toofar, unrendered (mask 0), one gross outlier; a buffer with packs of 1
    sample, one of 200, and rays absent from it"""
    g = torch.Generator().manual_seed(seed)
    ranges = 2.0 + 58.0 * torch.rand(N, generator=g)
    depth = ranges + (0.05 + 0.45 * torch.rand(N, generator=g)) * (torch.randint(0, 2, [N], generator=g) * 2 - 1).float()
    mask = 0.5 + 0.5 * torch.rand(N, generator=g)
    idx = torch.arange(N)
    if invalid_every:
        ranges[idx % invalid_every == 2] = 0.0
        ranges[idx % invalid_every == 4] = 90.0 + idx[idx % invalid_every == 4].float()
        mask[idx % invalid_every == 5] = 0.0
    if N > 10:
        depth[10] = ranges[10] + 70.0             # valid, and 350 x the median error: the median gate removes it
    hit = torch.tensor([i for i in range(N) if N < 3 or i % 5 != 3], dtype=torch.long)
    n = torch.randint(2, 13, [hit.shape[0]], generator=g)
    n[::3] = 1
    if hit.shape[0] > 1:
        n[1] = 200
    pi = torch.stack([torch.cumsum(n, 0) - n, n], dim=1)
    S = int(n.sum())
    seg = torch.repeat_interleave(torch.arange(hit.shape[0]), n)
    off = (torch.rand(S, generator=g) * 2 - 1) * 3.0 * (bound or 1.0)
    if bound is not None:
        off = torch.where((off.abs() - bound).abs() < 1e-2, off * 1.05 + 0.02, off)
    t = ranges[hit][seg] + off
    vw = torch.rand(S, generator=g)
    vw = vw / torch.zeros(hit.shape[0]).index_add(0, seg, vw)[seg] * 0.95
    vb = dict(type="packed", rays_inds_hit=hit, pack_infos_hit=pi, t=t, vw=vw)
    return depth, mask, ranges, vb


def _assert_margins(info, vb, ranges, bound):
    """the inputs keep their distance from every threshold: nothing here is decided by the last bit"""
    if info["thr"] is not None and float(info["thr"]) > 0:
        e, thr = info["err"][info["valid"]], float(info["thr"])
        assert bool(((e - thr).abs() > 1e-3 * thr).all())
    if bound is not None and vb["type"] != "empty":
        seg = torch.repeat_interleave(torch.arange(vb["pack_infos_hit"].shape[0]), vb["pack_infos_hit"][:, 1])
        d = (vb["t"] - ranges[vb["rays_inds_hit"]][seg]).abs()
        assert bool(((d - bound).abs() > 1e-4).all())


def _lidar_both(backend, depth, mask, ranges, vb, cfg, tag, far=None, mult=1.0, **kw):
    kw = dict(dict(discard_toofar=TOOFAR, discard_outliers_median=FACTOR), **kw)
    empty = vb["type"] == "empty"
    leaves = [depth] + ([] if empty else [vb["vw"]])
    infos = {}

    def fn_ref(dt, d, vw=None):
        out, info = ref.lidar(d, vw, dt, depth, mask, ranges, vb, depth_cfg=cfg.get("depth"), los_cfg=cfg.get("line_of_sight"),
                              far=far, **kw)
        infos[dt] = info
        return out

    def fn_op(d, vw=None):
        aux = {}
        out = losses.lidar_loss(dict(depth_volume=d, mask_volume=mask.to(backend)), vb if empty else _to(vb, backend, vw=vw),
                                ranges.to(backend), depth=cfg.get("depth"), line_of_sight=cfg.get("line_of_sight"), far=far, aux=aux,
                                **kw)
        infos["op"] = aux
        return out
    r32, r64 = _ref_run(fn_ref, leaves)
    info = infos[torch.float64]
    _assert_margins(info, vb, ranges, _los_bound(cfg))
    vals, grads = _op_run(fn_op, leaves, backend)
    aux = infos["op"]
    assert torch.equal(aux["valid"].cpu(), info["valid"]) and torch.equal(aux["keep"].cpu(), info["keep"])
    assert torch.equal(aux["err"].cpu(), info["err"])
    if info["median"] is not None:
        assert int(aux["median"].cpu().view(torch.int32)) == int(info["median"].view(torch.int32))
    if info["member"] is not None:
        assert torch.equal(aux["member"].cpu(), info["member"])
    _check(tag, vals, grads, r32, r64, mult=mult)
    return vals, grads, info


@pytest.mark.parametrize("ci", range(len(LIDAR_CFGS)))
@pytest.mark.parametrize("N", NS)
def test_lidar_matches_float64(backend, N, ci):
    cfg = LIDAR_CFGS[ci]
    depth, mask, ranges, vb = _lidar_case(N, 70 + N + ci, _los_bound(cfg))
    vals, grads, info = _lidar_both(backend, depth, mask, ranges, vb, cfg, f"lidar N={N} cfg{ci}", far=120.0)
    want = (["lidar_loss.depth"] if "depth" in cfg else []) + \
        ([] if "line_of_sight" not in cfg else (["lidar_loss.los.empty"] if cfg["line_of_sight"].get("fn_type", "nerf") == "neus_unisim"
                                                else ["lidar_loss.los.neighbor", "lidar_loss.los.empty"]))
    assert list(vals) == want
    if N == 300:                                  # what the case is made of
        v, k = info["valid"], info["keep"]
        assert not bool(v[ranges == 0].any()) and not bool(v[ranges > TOOFAR].any()) and not bool(v[mask == 0].any())
        assert bool(v[10]) and not bool(k[10]) and int(v.sum()) - int(k.sum()) == 1                  # the gross outlier, alone
        assert torch.equal(grads[0].cpu()[~k], torch.zeros(int((~k).sum())))
        absent = torch.ones(N, dtype=torch.bool)
        absent[vb["rays_inds_hit"]] = False
        assert bool(absent.any()) and bool((vb["pack_infos_hit"][:, 1] == 1).any()) and bool((vb["pack_infos_hit"][:, 1] == 200).any())


def test_lidar_reference_reading_of_the_range_gate(backend):
    """``toofar_replaces_mask=True``: line :266 as written -- the no-return beams and the unrendered ones count as valid"""
    cfg = LIDAR_CFGS[0]
    depth, mask, ranges, vb = _lidar_case(65, 81, 1.5)
    _, _, a = _lidar_both(backend, depth, mask, ranges, vb, cfg, "lidar default gate")
    _, _, b = _lidar_both(backend, depth, mask, ranges, vb, cfg, "lidar replaced gate", toofar_replaces_mask=True)
    assert not bool(a["valid"][ranges == 0].any()) and bool(b["valid"][ranges == 0].all()) and bool(b["valid"][mask == 0].all())
    assert torch.equal(b["valid"], ranges <= TOOFAR)
    _, _, c = _lidar_both(backend, depth, mask, ranges, vb, cfg, "lidar no range gate", discard_toofar=None, toofar_replaces_mask=True)
    assert torch.equal(c["valid"], (mask > 1e-7) & (ranges > 0))
    _, _, d = _lidar_both(backend, depth, mask, ranges, vb, cfg, "lidar no median gate", discard_outliers_median=0)
    assert torch.equal(d["keep"], d["valid"]) and d["median"] is None


def test_lidar_median_zero_discards_every_beam_with_an_error(backend):
    """more than half of the beams invalid: their error entries are 0, so is the median, and ``err > 0 * factor`` removes every
    valid beam whose prediction is not exact -- the reference does this, and so do the kernels"""
    N = 65
    depth, mask, ranges, vb = _lidar_case(N, 82, 1.5)
    ranges[:40] = 0.0
    depth[50] = ranges[50]                         # one exact prediction: error 0, not greater than 0, kept
    vb["t"] = vb["t"] + 0.0
    vals, grads, info = _lidar_both(backend, depth, mask, ranges, vb, LIDAR_CFGS[0], "lidar median 0")
    assert float(info["median"]) == 0.0 and int(info["valid"].sum()) < N // 2
    assert bool(info["valid"][50]) and torch.equal(info["keep"], info["valid"] & (info["err"] == 0)) and int(info["keep"].sum()) == 1
    assert float(vals["lidar_loss.depth"].detach()) == 0.0 and torch.equal(grads[0].cpu(), torch.zeros(N))


def test_lidar_ties_go_the_way_the_comparisons_are_written(backend):
    """exactly representable values ON the thresholds: ``>`` and ``<`` strict, ``<=`` and ``>=`` inclusive"""
    # beams: 0 err = median x factor exactly; 1 err the next float above; 2 range == discard_toofar; 3 mask == thresh; 4..6 median
    ranges = torch.tensor([1.0, 1.0, 80.0, 1.0, 1.0, 1.0, 1.0])
    depth = torch.tensor([1.0 + 25.0, 0.0, 80.25, 1.25, 1.25, 1.25, 1.25])
    depth[1] = 1.0 + torch.nextafter(torch.tensor(25.0), torch.tensor(100.0))
    thresh = ref.f32(1e-7)
    mask = torch.tensor([1.0, 1.0, 1.0, thresh, 1.0, 1.0, 1.0])
    hit = torch.arange(7)
    t = torch.tensor([2.5, -0.5, 2.5 + 2.0 ** -20, -0.5 - 2.0 ** -20, 1.0])               # beam 0: gt 1.0, bound 1.5
    n = torch.tensor([5, 1, 1, 1, 1, 1, 1])
    pi = torch.stack([torch.cumsum(n, 0) - n, n], 1)
    tt = torch.cat([t, ranges[1:] + 0.25])
    vb = dict(type="packed", rays_inds_hit=hit, pack_infos_hit=pi, t=tt, vw=torch.linspace(0.1, 0.6, 11))
    kw = dict(discard_toofar=80.0, discard_outliers_median=100.0, mask_pred_thresh=1e-7)
    for cfg, want in ((dict(depth=dict(fn_type="l1"), line_of_sight=dict(fn_type="neus_unisim", fn_param=dict(epsilon=1.5))), [0, 0, 2, 2, 0]),
                      (dict(depth=dict(fn_type="l1"), line_of_sight=dict(fn_type="nerf", fn_param=dict(sigma=1.5))), [1, 1, 0, 2, 1])):
        infos = {}
        out = losses.lidar_loss(dict(depth_volume=depth.to(backend), mask_volume=mask.to(backend)), _to(vb, backend), ranges.to(backend),
                                aux=infos, **cfg, **kw)
        sync(backend)
        _, info = ref.lidar(depth.double(), vb["vw"].double(), torch.float64, depth, mask, ranges, vb, depth_cfg=cfg["depth"],
                            los_cfg=cfg["line_of_sight"], **kw)
        assert float(info["median"]) == 0.25 and float(info["thr"]) == 25.0
        assert info["valid"].tolist() == [True, True, True, False, True, True, True]             # 80 <= 80; thresh > thresh is false
        assert info["keep"].tolist() == [True, False, True, False, True, True, True]             # 25 > 25 is false; the next float is
        assert info["member"][:5].tolist() == want
        assert torch.equal(infos["valid"].cpu(), info["valid"]) and torch.equal(infos["keep"].cpu(), info["keep"])
        assert torch.equal(infos["member"].cpu(), info["member"])
        assert all(math.isfinite(float(v)) for v in out.values())


def test_lidar_empty_buffer_and_refusals(backend):
    depth, mask, ranges, vb = _lidar_case(64, 83, 1.5)
    vals, _, _ = _lidar_both(backend, depth, mask, ranges, dict(type="empty"), LIDAR_CFGS[0], "lidar empty buffer")
    assert list(vals) == ["lidar_loss.depth"]
    rd = dict(depth_volume=depth.to(backend), mask_volume=mask.to(backend))
    r, b = ranges.to(backend), _to(vb, backend)
    with pytest.raises(NotImplementedError, match="discard_outliers"):
        losses.lidar_loss(rd, b, r, depth=dict(fn_type="l1"), discard_outliers=0.1)
    with pytest.raises(NotImplementedError, match="fn_type"):
        losses.lidar_loss(rd, b, r, depth=dict(fn_type="l3"))
    with pytest.raises(NotImplementedError, match="type"):
        losses.lidar_loss(rd, dict(b, type="batched"), r, line_of_sight=dict(fn_type="nerf"))
    with pytest.raises(TypeError, match="epsilon"):
        losses.lidar_loss(rd, b, r, line_of_sight=dict(fn_type="nerf", fn_param=dict(epsilon=1.0)))
    with pytest.raises(TypeError, match="weight"):
        losses.lidar_loss(rd, b, r, depth=dict(weight=1.0))
    with pytest.raises(TypeError):
        losses.lidar_loss(rd, b, r, discard_nearer=1.0)
    with pytest.raises(ValueError, match="far"):
        losses.lidar_loss(rd, b, r, depth=dict(fn_type="l2_normalized"))


def test_lidar_anneals_resolve_on_the_host(backend):
    """the yaml's epsilon_anneal (milestones [5000, 10000], vals [1.5, 0.75, 0.5]) and a linear weight anneal"""
    depth, mask, ranges, vb = _lidar_case(64, 84, None)
    los = dict(w=0.1, fn_type="neus_unisim", fn_param=dict(epsilon_anneal=dict(type="milestones", milestones=[5000, 10000], vals=[1.5, 0.75, 0.5])))
    dep = dict(fn_type="l1", anneal=dict(type="linear", start_it=0, stop_it=1000, start_val=0.0, stop_val=0.02))
    seen = []
    for it, eps, w in ((0, 1.5, 0.0), (4999, 1.5, 0.02), (5000, 0.75, 0.02), (9999, 0.75, 0.02), (10000, 0.5, 0.02), (500, 1.5, 0.01)):
        aux = {}
        out = losses.lidar_loss(dict(depth_volume=depth.to(backend), mask_volume=mask.to(backend)), _to(vb, backend), ranges.to(backend),
                                depth=dep, line_of_sight=los, it=it, aux=aux)
        assert aux["epsilon"] == eps
        o64, _ = ref.lidar(depth.double(), vb["vw"].double(), torch.float64, depth, mask, ranges, vb, depth_cfg=dict(fn_type="l1", w=w),
                           los_cfg=dict(w=0.1, fn_type="neus_unisim", fn_param=dict(epsilon=eps)))
        for k in o64:
            assert abs(float(out[k]) - float(o64[k])) <= 1e-5 * abs(float(o64[k])) + 1e-12, (it, k)
        seen.append(float(out["lidar_loss.los.empty"]))
    assert seen[0] < seen[2] < seen[4]              # a narrower neighbourhood leaves more of the ray outside it


# ------------------------------------------------------------------------------------------------ 6. launch budget
def _count(monkeypatch, fn):
    monkeypatch.setattr(_lib, "CALL_COUNT", 0)
    out = fn()
    n = _lib.CALL_COUNT
    monkeypatch.setattr(_lib, "CALL_COUNT", None)
    return out, n


def test_launch_budget(backend, monkeypatch):
    """C-ABI calls per direction: lidar 3 + 1, every other loss 1 + 1 (the entropy without ``object_mask_in_total``)"""
    N = 64
    depth, mask, ranges, vb = _lidar_case(N, 85, 1.5)
    pred, gt = _mask_inputs(N, MASK_CFGS[0], 86)
    x = torch.randn(257) * 0.05
    cases = {
        "lidar": (3, lambda d, w: sum(losses.lidar_loss(dict(depth_volume=d, mask_volume=mask.to(backend)), _to(vb, backend, vw=w),
                                                        ranges.to(backend), discard_toofar=80.0, **LIDAR_CFGS[1]).values()), [depth, vb["vw"]]),
        "mask": (1, lambda p: losses.mask_occupancy_loss(p, gt.to(backend), safe_bce=True, pred_clip=0)[0], [pred]),
        "sparsity": (1, lambda v: losses.sparsity_loss(v, inv_scale=16.0, w=0.1), [x]),
        "clearance": (1, lambda v: losses.clearance_loss(v, beta=10.0, thresh=0.01), [x]),
        "entropy": (1, lambda a, b: sum(losses.mask_entropy_loss("cross_crdv", mask_cr=a, mask_dv=b).values()), [pred, gt * 0.5 + 0.2]),
    }
    for name, (fwd_max, fn, inputs) in cases.items():
        ls = [leaf(t, backend) for t in inputs]
        loss, n_fwd = _count(monkeypatch, lambda: fn(*ls))
        _, n_bwd = _count(monkeypatch, loss.backward)
        sync(backend)
        print(f"{name}: {n_fwd} C-ABI calls forward, {n_bwd} backward")
        assert 1 <= n_fwd <= fwd_max and n_bwd == 1, (name, n_fwd, n_bwd)
        assert all(t.grad is not None and float(t.grad.abs().max()) > 0 for t in ls)


# ------------------------------------------------------------------------------------------------ 7. trainer
def _street_trainer(backend, loss_cfg, **kw):
    from neuralsim_amd import scenarios as sc
    return sc.build_street_trainer(backend, small=True, rays_per_gpu=48, lidar_rays=48, num_uniform=16, loss_cfg=loss_cfg, **kw)


def _spy(tr, monkeypatch):
    """records what the two steps of one iteration hand to their losses: (ret, aux) of the pixel step, (ret, ranges, uniform
    samples, epsilon) of the lidar step"""
    seen = {}
    loss, render, sample, uniform, lidar_loss = tr.loss, tr.renderer.render, tr.sample_lidar_batch, tr.model.sample_pts_uniform, losses.lidar_loss

    def weights():          # the regularised tensors as they are when a step's losses are formed
        return {c: [(p.detach().cpu().clone(), p is getattr(mod, "rad_w", None)) for p in mod._weight_reg_tensors()]
                for c, mod in (("Street", tr.model), ("Distant", tr.distant_model))}

    def loss_(ret, gt, uni=None, aux=None):
        seen["pixel"], seen["w_pixel"] = (ret, aux), weights()
        return loss(ret, gt, uni, aux=aux)

    def render_(*a, **k):
        seen["ret"] = render(*a, **k)
        return seen["ret"]

    def sample_():
        seen["beams"] = sample()
        return seen["beams"]

    def uniform_(*a, **k):
        seen["uni"] = uniform(*a, **k)
        return seen["uni"]

    def lidar_loss_(*a, **k):
        aux = {}
        out = lidar_loss(*a, aux=aux, **k)
        seen["lidar_aux"], seen["w_lidar"] = aux, weights()
        return out
    tr.loss, tr.renderer.render, tr.sample_lidar_batch, tr.model.sample_pts_uniform = loss_, render_, sample_, uniform_
    monkeypatch.setattr(losses, "lidar_loss", lidar_loss_)
    return seen


def _cpu(x):
    if torch.is_tensor(x):
        return x.detach().cpu()
    if isinstance(x, dict):
        return {k: _cpu(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return type(x)(_cpu(v) for v in x)
    return x


def _close(tag, got, fn):
    """fn(dtype) -> the restatement's value; the bound of this file on one number"""
    v32, v64 = float(fn(torch.float32)), float(fn(torch.float64))
    tol = max(MARGIN * abs(v32 - v64), FLOOR * abs(v64))
    print(f"{tag}: {float(got):.7e} err {abs(float(got) - v64):.2e} (f32 torch {abs(v32 - v64):.2e}, bound {tol:.2e})")
    assert math.isfinite(float(got)) and abs(float(got) - v64) <= tol, (tag, float(got), v64, tol)


def _weight_reg(tensors, skip_radiance):
    return lambda dt: sum(p.to(dt).norm(p=2.0) for p, is_rad in tensors if not (skip_radiance and is_rad))


def test_trainer_street_loss_cfg(backend, monkeypatch):
    """the yaml's blocks on the small street scenario: every configured key is there, finite, and equal to the restatement applied
    to the SAME render; mask_entropy and sparsity wait for their ``enable_after``; the line-of-sight epsilon follows its milestones"""
    import copy
    from neuralsim_amd import scenarios as sc
    from nr3d_lib.models.annealers import get_anneal_val
    cfg = copy.deepcopy(sc.STREET_LOSS_CFG)
    cfg["mask_entropy"].update(enable_after=2, anneal=dict(type="linear", start_it=1, stop_it=3, start_val=0, stop_val=0.005))
    cfg["sparsity"]["enable_after"] = 1
    cfg["sparsity"]["class_name_cfgs"]["Street"]["anneal"].update(start_it=0, stop_it=2, update_every=1)
    cfg["lidar"]["line_of_sight"]["fn_param"]["epsilon_anneal"]["milestones"] = [1, 2]
    tr = _street_trainer(backend, cfg)
    assert not tr._fused_ok() and tr.target_masks.shape == tr.target_images.shape[:3]
    assert set(tr.target_masks.unique().tolist()) <= {0.0, 1.0} and 0.0 < float(tr.target_masks.mean()) < 1.0
    seen = _spy(tr, monkeypatch)
    m, dm = tr.model, tr.distant_model
    sp_cfg = cfg["sparsity"]["class_name_cfgs"]["Street"]
    for it, eps in ((0, 1.5), (1, 0.75), (2, 0.5)):
        tr.train_step(it)
        sync(backend)
        parts, lparts = tr.loss_parts, tr._lidar_parts
        want = {"loss_rgb", "loss_eikonal", "loss_mask", "loss_clearance.Street", "loss_weight_reg.Street", "loss_weight_reg.Distant"}
        want |= ({"loss_sparsity.Street"} if it >= 1 else set()) | ({"loss_mask_entropy.crisp_cr"} if it >= 2 else set())
        assert set(parts) == want, (it, sorted(parts))
        lwant = {"lidar_loss.depth", "lidar_loss.los.empty", "eikonal_render", "loss_clearance.Street", "loss_weight_reg.Street",
                 "loss_weight_reg.Distant"} | ({"loss_sparsity.Street"} if it >= 1 else set())
        assert set(lparts) == lwant, (it, sorted(lparts))
        assert all(torch.is_tensor(v) and not v.requires_grad and v.device.type == backend.type and math.isfinite(float(v))
                   for v in list(parts.values()) + list(lparts.values()))
        assert seen["lidar_aux"]["epsilon"] == eps
        # ---- the pixel step's terms, restated on its own render
        ret, aux = _cpu(seen["pixel"][0]), _cpu(seen["pixel"][1])
        raw, N = ret["raw_per_obj_model"], ret["rendered"]["mask_volume"].shape[0]
        mv = ret["rendered"]["mask_volume"]
        _close(f"it {it} loss_mask", parts["loss_mask"],
               lambda dt: ref.mask_occupancy(mv.to(dt), aux["mask"], dt, safe_bce=True, pred_clip=0, w=0.3)[0])
        assert raw["main"]["volume_buffer"]["type"] != "empty"
        near = raw["main"]["details"]["near_sdf"]
        th = ref.f32(0.02)
        _close(f"it {it} loss_clearance", parts["loss_clearance.Street"], lambda dt: ref.clearance(near.to(dt), near < 0.02, 10.0, th, w=0.2))
        _close(f"it {it} loss_weight_reg.Street", parts["loss_weight_reg.Street"], lambda dt: 1e-6 * _weight_reg(seen["w_pixel"]["Street"], False)(dt))
        _close(f"it {it} loss_weight_reg.Distant", parts["loss_weight_reg.Distant"], lambda dt: 1e-6 * _weight_reg(seen["w_pixel"]["Distant"], False)(dt))
        w_sp = get_anneal_val(it=it, **sp_cfg["anneal"])
        if it >= 1:
            sdf = raw["main"]["extra_pts"]["sdf"]
            assert sdf.shape[0] == 16
            _close(f"it {it} loss_sparsity", parts["loss_sparsity.Street"], lambda dt: ref.sparsity(sdf.to(dt), inv_scale=16.0, w=w_sp))
        if it >= 2:
            w_en = get_anneal_val(it=it, **cfg["mask_entropy"]["anneal"])
            assert w_en > 0
            _close(f"it {it} loss_mask_entropy", parts["loss_mask_entropy.crisp_cr"],
                   lambda dt: ref.mask_entropy("crisp_cr", dt, mask_cr=ref.object_mask_in_total(raw["main"]["volume_buffer"], N, dt),
                                               eps=ref.f32(1e-5), w=w_en)["loss_mask_entropy.crisp_cr"])
        # ---- the lidar step's
        lret, (_, _, ranges) = _cpu(seen["ret"]), _cpu(seen["beams"])
        vb, rd = lret["volume_buffer"], lret["rendered"]
        assert vb["type"] == "packed"
        for key in ("lidar_loss.depth", "lidar_loss.los.empty"):
            _close(f"it {it} {key}", lparts[key], lambda dt: ref.lidar(
                rd["depth_volume"].to(dt), vb["vw"].to(dt), dt, rd["depth_volume"], rd["mask_volume"], ranges, vb,
                depth_cfg=dict(w=0.02, fn_type="l1"), los_cfg=dict(w=0.1, fn_type="neus_unisim", fn_param=dict(epsilon=eps)),
                discard_toofar=80.0, discard_outliers_median=100.0)[0][key])
        lnear = lret["raw_per_obj_model"]["main"]["details"]["near_sdf"]
        _close(f"it {it} lidar loss_clearance", lparts["loss_clearance.Street"], lambda dt: ref.clearance(lnear.to(dt), lnear < 0.02, 10.0, th, w=0.2))
        _close(f"it {it} lidar loss_weight_reg.Street", lparts["loss_weight_reg.Street"], lambda dt: 1e-6 * _weight_reg(seen["w_lidar"]["Street"], True)(dt))
        if it >= 1:
            lsdf = _cpu(seen["uni"]["sdf"])
            _close(f"it {it} lidar loss_sparsity", lparts["loss_sparsity.Street"], lambda dt: ref.sparsity(lsdf.to(dt), inv_scale=16.0, w=w_sp))
        want_total = sum(float(v) for v in lparts.values())
        assert abs(float(tr._loss_lidar) - want_total) <= 1e-5 * (1 + abs(want_total))


def test_trainer_street_lidar_step_touches_only_the_parameters_of_its_graph(backend):
    """``test_lidar_step_touches_only_the_parameters_of_its_graph`` (tests/test_trainer.py) for the ``loss_cfg`` path: the lidar
    render runs with ``with_rgb=False``, and its weight regulariser covers the tensors of its graph only -- radiance, appearance
    and sky parameters keep their value, their Adam moments and their step count; the SDF side is stepped twice per iteration"""
    from neuralsim_amd import scenarios as sc
    tr = _street_trainer(backend, sc.STREET_LOSS_CFG)
    m, dm, sm = tr.model, tr.distant_model, tr.sky_model
    tr._train_step_pixel(0)
    grp = {id(g["p"]): g for g in tr.optim.groups}
    lidar_free = [m.rad_w, m.rad_b, tr.appear, dm.rad_w, dm.rad_b, sm.w, sm.b]
    in_graph = [m.encoding.flattened_params, m.sdf_w, m.sdf_b, dm.flattened_params, dm.den_w, dm.den_b]
    assert all(grp[id(p)]["t"] == 1 for p in lidar_free + in_graph)
    snap = [(p.detach().clone(), grp[id(p)]["m"].clone(), grp[id(p)]["v"].clone()) for p in lidar_free]
    before = [p.detach().clone() for p in in_graph]
    loss = tr.train_step_lidar(0)
    sync(backend)
    assert math.isfinite(float(loss)) and tr.stats["lidar_samples"] > 0
    parts = tr._lidar_parts
    assert float(parts["lidar_loss.depth"]) > 0 and float(parts["lidar_loss.los.empty"]) >= 0 and float(parts["eikonal_render"]) > 0
    assert abs(float(loss) - sum(float(v) for v in parts.values())) < 1e-5 * (1 + abs(float(loss)))
    for p, (p0, m0, v0) in zip(lidar_free, snap):
        g = grp[id(p)]
        assert p.grad is None and g["t"] == 1
        assert torch.equal(p.detach(), p0) and torch.equal(g["m"], m0) and torch.equal(g["v"], v0)
    for p, p0 in zip(in_graph, before):
        assert grp[id(p)]["t"] == 2 and not torch.equal(p.detach(), p0)


def test_trainer_without_loss_cfg_is_bit_identical(backend):
    """a street trainer built by the parent's signature and one handed ``loss_cfg=None`` explicitly (which the scenario passes on to
    ``RenderTrainer(loss_cfg=None, target_masks=None)``): the same path, the same terms, the same losses and parameters over three
    iterations (pixel + lidar).  Exactly on the emulator; on the device two runs of ONE trainer differ by the order of their float
    atomics, and the two are held to the allowance ``test_trainer_without_the_term_is_bit_identical`` of tests/test_s3im.py gives
    such runs."""
    from neuralsim_amd import scenarios as sc
    outs = []
    for kw in (dict(), dict(loss_cfg=None)):
        torch.manual_seed(1234)          # (the scenario initialises its models from the global generator)
        tr = sc.build_street_trainer(backend, small=True, rays_per_gpu=48, lidar_rays=48, num_uniform=16, **kw)
        assert tr.loss_cfg is None and tr.target_masks is None
        ls = []
        for it in range(3):
            ls += [float(tr.train_step(it)), float(tr._loss_lidar)]
        sync(backend)
        assert sorted(tr.loss_parts) == ["loss_eikonal", "loss_rgb"] and sorted(tr._lidar_parts) == ["depth", "eikonal_render", "los"]
        assert all(isinstance(v, float) for v in tr._lidar_parts.values())
        outs.append((ls, [p.detach().cpu().clone() for p in tr.optim.params()], tr.gen.get_state().cpu()))
    a, b = outs
    assert all(math.isfinite(l) for l in a[0]) and torch.equal(a[2], b[2])
    if backend.type != "cuda":
        assert a[0] == b[0] and all(torch.equal(p, q) for p, q in zip(a[1], b[1]))
        return
    assert all(abs(x - y) <= 1e-5 * (1 + abs(x)) for x, y in zip(a[0], b[0])), (a[0], b[0])
    for p, q in zip(a[1], b[1]):
        d = (p.float() - q.float()).abs()
        bad = d > (5e-5 + 1e-4 * p.float().abs())
        assert float(bad.float().mean()) < 2e-3 and float(d.max()) <= 2 * 3 * 2 * 1e-3      # 3 iterations x 2 steps x lr


def test_trainer_loss_cfg_refusals(backend):
    from neuralsim_amd import scenarios as sc
    with pytest.raises(NotImplementedError, match="ray_vw_entropy"):
        _street_trainer(backend, dict(ray_vw_entropy=dict(w=1.0)))
    with pytest.raises(NotImplementedError, match="Distant"):
        _street_trainer(backend, dict(clearance=dict(class_name_cfgs=dict(Distant=dict(w=1.0)))))
    with pytest.raises(NotImplementedError, match="mode"):
        _street_trainer(backend, dict(mask_entropy=dict(w=1.0, mode="crisp_sky")))
    tr = _street_trainer(backend, dict(clearance=0.2, weight_reg=1e-6))      # a bare number: every class (clearance.py:43-44)
    assert tr.loss_cfg["weight_reg"]["class_name_cfgs"] == dict(Street=dict(w=1e-6), Distant=dict(w=1e-6))
    assert sc.STREET_LOSS_CFG["clearance"]["class_name_cfgs"]["Street"]["w"] == 0.2


# ------------------------------------------------------------------------------------------------ 8. the reference's own classes
# tests/golden/make_street_loss_fixture.py runs MaskOccupancyLoss, MaskEntropyRegLoss.forward_code_single, SparsityLoss,
# ClearanceLoss and LidarLoss (loaded unchanged through ref_glue.reference_loss_module, on the emulator) on these inputs and
# freezes inputs, losses and gradients; the replay runs this package's ops on both backends against the frozen float32 run.
FIX_N = 65
FIX_MASK = dict(w=0.3, safe_bce=True, pred_clip=0)                                    # the yaml
FIX_ENTROPY = dict(crisp_cr=dict(w=0.005, mode="crisp_cr"), cross_crdv_detached=dict(w=0.01, mode="cross_crdv_detached"))
FIX_SPARSITY = dict(key="sdf", type="normalized_logistic_density", inv_scale=16.0, w=2.0e-3)
FIX_CLEARANCE = dict(w=0.2, beta=10.0, thresh=0.02)
FIX_LIDAR = dict(
    unisim=dict(depth=dict(w=0.02, fn_type="l1", fn_param={}), line_of_sight=dict(w=0.1, fn_type="neus_unisim", fn_param=dict(epsilon=1.5)),
                discard_toofar=80.0, discard_outliers_median=100.0),
    nerf=dict(depth=dict(w=0.02, fn_type="l1_log", fn_param={}),
              line_of_sight=dict(w=0.1, fn_type="nerf", fn_param=dict(sigma=1.5, sigma_scale_factor=3.0)),
              discard_toofar=80.0, discard_outliers_median=100.0))


def fixture_inputs():
    pred, gt = _mask_inputs(FIX_N, FIX_MASK, 901)
    g = torch.Generator().manual_seed(902)
    depth, mask, ranges, vb = _lidar_case(FIX_N, 903, 1.5)
    # a batch in which both readings of lidar.py:266 coincide: every beam returns and is rendered (some of them beyond toofar)
    depth2, _, ranges2, vb2 = _lidar_case(FIX_N, 904, 1.5, invalid_every=0)
    ranges2[::9] = 85.0 + torch.arange(ranges2[::9].shape[0]).float()
    depth2[::9] = ranges2[::9] + 0.2
    seg = torch.repeat_interleave(torch.arange(vb2["pack_infos_hit"].shape[0]), vb2["pack_infos_hit"][:, 1])
    g2 = torch.Generator().manual_seed(905)
    off = (torch.rand(seg.shape[0], generator=g2) * 2 - 1) * 4.5
    vb2["t"] = ranges2[vb2["rays_inds_hit"]][seg] + torch.where((off.abs() - 1.5).abs() < 1e-2, off * 1.05 + 0.02, off)
    return dict(mask_pred=pred, mask_gt=gt, cr=_packed_object(FIX_N, 906), dv=_distant_object(FIX_N, 5, 907),
                sdf=torch.randn(257, generator=g) * 0.2, near_sdf=torch.randn(257, generator=g) * 0.05,
                lidar=dict(depth=depth, mask=mask, ranges=ranges, vb=vb),
                lidar_all_return=dict(depth=depth2, mask=torch.full([FIX_N], 0.9), ranges=ranges2, vb=vb2))


def _replay(tag, backend, fn_op, fn_ref, leaves, frozen_vals, frozen_grads):
    """this package's op against the frozen float32 run of the reference's class: twice the bound of the file (both lie within
    one bound of the float64 restatement, which the op is held to as well)"""
    r32, r64 = _ref_run(fn_ref, leaves)
    vals, grads = _op_run(fn_op, leaves, backend)
    _check(f"{tag} vs float64", vals, grads, r32, r64)
    assert list(vals) == list(frozen_vals), (tag, list(vals), list(frozen_vals))
    _check(f"{tag} vs the reference's run", vals, grads, r32, r64, mult=2.0,
           target=({k: v.double() for k, v in frozen_vals.items()}, [g.double() for g in frozen_grads]))


def test_reference_classes_replayed_from_the_fixture(backend):
    fx = torch.load(FIXTURE)
    inp, out = fx["inputs"], fx["outputs"]
    mine = fixture_inputs()
    assert torch.equal(inp["mask_pred"], mine["mask_pred"]) and torch.equal(inp["lidar"]["depth"], mine["lidar"]["depth"])
    assert torch.equal(inp["lidar_all_return"]["vb"]["t"], mine["lidar_all_return"]["vb"]["t"]) and torch.equal(inp["sdf"], mine["sdf"])
    N = FIX_N
    for mode in (None, "always_occupied", "only_cull_non_occupied", "only_preserve_occupied"):
        fr = out[f"mask.{mode}"]
        kw = dict(FIX_MASK, special_mask_mode=mode)
        holder = {}

        def run(p):
            loss, holder["err"] = losses.mask_occupancy_loss(p, inp["mask_gt"].to(backend), **kw)
            return {"loss_mask": loss}
        _replay(f"MaskOccupancyLoss {mode}", backend, run, lambda dt, p: {"loss_mask": ref.mask_occupancy(p, inp["mask_gt"], dt, **kw)[0]},
                [inp["mask_pred"]], fr["losses"], fr["grads"])
        assert torch.equal(holder["err"].cpu(), fr["err"])
    for name, cfg in FIX_ENTROPY.items():
        fr = out[f"entropy.{name}"]

        def run(vcr, vdv):
            return losses.mask_entropy_loss(cfg["mode"], w=cfg["w"], mask_cr=losses.object_mask_in_total(_to(inp["cr"], backend, vw_in_total=vcr), N),
                                            mask_dv=losses.object_mask_in_total(_to(inp["dv"], backend, vw_in_total=vdv), N))
        _replay(f"MaskEntropyRegLoss {name}", backend, run, lambda dt, vcr, vdv: ref.mask_entropy(
            cfg["mode"], dt, mask_cr=ref.object_mask_in_total(dict(inp["cr"], vw_in_total=vcr), N, dt),
            mask_dv=ref.object_mask_in_total(dict(inp["dv"], vw_in_total=vdv), N, dt), eps=ref.f32(1e-5), w=cfg["w"]),
            [inp["cr"]["vw_in_total"], inp["dv"]["vw_in_total"]], fr["losses"], fr["grads"])
    sp = {k: v for k, v in FIX_SPARSITY.items() if k not in ("key", "type")}
    _replay("SparsityLoss", backend, lambda x: {"loss_sparsity.Street": losses.sparsity_loss(x, FIX_SPARSITY["type"], **sp)},
            lambda dt, x: {"loss_sparsity.Street": ref.sparsity(x, FIX_SPARSITY["type"], **sp)}, [inp["sdf"]],
            out["sparsity"]["losses"], out["sparsity"]["grads"])
    below = inp["near_sdf"] < FIX_CLEARANCE["thresh"]
    _replay("ClearanceLoss", backend, lambda x: {"loss_clearance.Street": losses.clearance_loss(x, **FIX_CLEARANCE)},
            lambda dt, x: {"loss_clearance.Street": ref.clearance(x, below, FIX_CLEARANCE["beta"], ref.f32(FIX_CLEARANCE["thresh"]), FIX_CLEARANCE["w"])},
            [inp["near_sdf"]], out["clearance"]["losses"], out["clearance"]["grads"])
    for case, replaces in (("lidar", True), ("lidar_all_return", False)):
        c = inp[case]
        for name, cfg in FIX_LIDAR.items():
            fr = out[f"{case}.{name}"]
            kw = dict(discard_toofar=cfg["discard_toofar"], discard_outliers_median=cfg["discard_outliers_median"], toofar_replaces_mask=replaces)
            infos = {}

            def run(d, vw):
                aux = {}
                o = losses.lidar_loss(dict(depth_volume=d, mask_volume=c["mask"].to(backend)), _to(c["vb"], backend, vw=vw),
                                      c["ranges"].to(backend), depth=cfg["depth"], line_of_sight=cfg["line_of_sight"], aux=aux, **kw)
                infos["op"] = aux
                return o

            def run_ref(dt, d, vw):
                o, infos[dt] = ref.lidar(d, vw, dt, c["depth"], c["mask"], c["ranges"], c["vb"], depth_cfg=cfg["depth"],
                                         los_cfg=cfg["line_of_sight"], **kw)
                return o
            _replay(f"LidarLoss {case} {name}", backend, run, run_ref, [c["depth"], c["vb"]["vw"]], fr["losses"], fr["grads"])
            info = infos[torch.float64]
            _assert_margins(info, c["vb"], c["ranges"], 1.5)
            assert torch.equal(infos["op"]["keep"].cpu(), info["keep"]) and torch.equal(infos["op"]["member"].cpu(), info["member"])
            assert torch.equal(infos["op"]["keep"].cpu(), fr["keep"])                 # the mask the reference's class ended with
            if case == "lidar_all_return":      # ... and there the literal reading gives the same mask
                alt, _ = ref.lidar_valid(c["depth"], c["mask"], c["ranges"], discard_toofar=80.0, toofar_replaces_mask=True)
                assert torch.equal(alt, info["valid"]) and not bool(info["valid"].all()) and int(info["keep"].sum()) > FIX_N // 2
