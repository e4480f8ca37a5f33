"""The monocular depth / normal cue losses (app/loss/mono.py): ``neuralsim_amd.losses.{mono_remain_mask,
mono_depth_ssi_loss, mono_depth_pearson_loss, mono_normal_cue_loss, packed_share}``, their C-ABI launch budget, the per-object share
of ``SingleVolumeRenderer``, ``RenderTrainer(loss_cfg=dict(mono_depth=, mono_normals=))`` and the replay of the reference's own
classes from tests/golden/mono_loss_fixture.pt -- against the restatement tests/mono_loss_ref.py.

Bounds (the project's own, as tests/test_street_losses.py).  Every case evaluates the restatement twice on the CPU, in float64 (the
reference value) and in float32 torch ops.  The kernels are allowed 8 x that float32 run's departure from float64 -- in a value,
|v - v64|, in a gradient or a per-ray image, max |g - g64| / max |g64| -- with a floor of 1e-6 relative; no element is exempt.
Against the frozen float32 run of the reference's classes the allowance is doubled.  The remain mask is compared exactly: the random
inputs keep ``mask_pred`` 1e-3 away from its threshold and the depths 1e-3 (relative) away from far, 0.8 far and the mean of the
prior (asserted on the inputs first), and one case puts exactly representable values ON every threshold.

Cases of the depth loss.  Up to 17x33 every fn_type runs the full product of scale_gt_to_pred x detach_scale_shift x grad_reg_scales
{0 (alpha 0), 1, 4} x pre-scale/shift {(1, 0), (50, 1)} x mask {ones, random 60 %, one pixel, empty} (``scale_gt_to_pred`` is left
out where det == 0: the reference divides by zero there).  At 64x64 and 80x120 the emulator needs ~0.1 s per case, so every fn_type
runs a rotation of eight combinations in which every value of every option occurs (``_rotation``); nothing in the kernels
depends on the image size beyond the number of workgroups and the sub-image strides, which those sizes exercise for every option.

Measured departures of the float32 CPU run from float64 over the cases of this file and the kernels' own, on the emulator (the
largest of each over the cases; values relative to |v64|, gradients to max |g64|):

    op                 f32 torch value   f32 torch grad    kernel value   kernel grad
    ssi depth          1.4e-04           1.8e-04           5.8e-07        9.4e-07
    pearson depth      2.7e-05           8.4e-06           1.3e-06        3.0e-07
    normal cue         1.6e-07           2.2e-07           5.1e-08        1.9e-07
    packed share       5.2e-07           4.3e-07           4.8e-08        1.2e-07

(``test_zz_measured_departures`` prints the table.  A Pearson term of a perfect correlation is ~0: its departures are taken relative
to the term's unit w alpha instead.)  The kernels sum in float64 and round once, so against float64 they sit at the float32 rounding
of their outputs where the float32 torch run carries the cancellation of the 2x2 solve (1e-4 on the 1-wide and 2x2 images) and of
the centred moments; the kernel columns' largest entries are the replay's, whose target is the reference's own float32 run."""
import math
from pathlib import Path

import pytest
import torch

import mono_loss_ref as ref
from conftest import sync
from neuralsim_amd import _lib, losses
from util import leaf

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = ROOT / "tests" / "golden" / "mono_loss_fixture.pt"
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 9), (16, 16), (17, 33), (64, 64), (80, 120)]
SMALL = [s for s in SHAPES if s[0] * s[1] <= 17 * 33]
NS = [1, 63, 64, 65, 300]
FLOOR, MARGIN = 1e-6, 8.0
COEF = (1.0, 0.7, 1.3, 0.4)     # upstream gradients of the returned terms: each its own
WORST = {}                      # op -> [f32 value, f32 grad, kernel value, kernel grad]: printed by the last test of each op


def _note(op, col, v):
    w = WORST.setdefault(op, [0.0, 0.0, 0.0, 0.0])
    w[col] = max(w[col], v)


def _check(op, tag, vals, grads, r32, r64, mult=1.0, target=None, unit=0.0):
    """vals: list of 0-dim tensors or per-ray images; grads: list of tensors; r32 / r64: (values, gradients) of the restatement,
    which set the bound; ``target`` (default r64): what the values and gradients are compared with.  ``unit``: the natural size of a
    value that may itself be ~0 (1 - r of a perfect correlation), for the table of measured departures only -- never for the bound"""
    target = r64 if target is None else target
    assert len(vals) == len(r64[0]), (tag, len(vals), len(r64[0]))
    for k, v in enumerate(vals):
        v64, v32, vt = r64[0][k].double(), r32[0][k].double(), target[0][k].double()
        assert v.dtype == torch.float32 and v.shape == v64.shape, (tag, k, v.shape, v64.shape)
        got = v.detach().cpu().double()
        scale = float(v64.abs().max()) if v64.numel() else 0.0
        e32, e = float((v32 - v64).abs().max()), float((got - vt).abs().max())
        tol = mult * max(MARGIN * e32, FLOOR * scale)
        print(f"{tag} value {k}: err {e:.2e} (f32 torch {e32:.2e}, bound {tol:.2e}, scale {scale:.2e})")
        assert bool(torch.isfinite(got).all()) and e <= tol, (tag, k, e, tol)
        if max(scale, unit) > 0:
            _note(op, 0, e32 / max(scale, unit)), _note(op, 2, e / max(scale, unit))
    assert len(grads) == len(r64[1])
    for j, (g, g32, g64) in enumerate(zip(grads, r32[1], r64[1])):
        assert g is not None and g.shape == g64.shape and bool(torch.isfinite(g).all()), (tag, j)
        if g64.numel() == 0:
            continue
        scale = float(g64.abs().max())
        e = float((g.detach().cpu().double() - target[1][j].double()).abs().max())
        if scale == 0.0:
            assert e == 0.0, (tag, j, e)
            continue
        e32 = float((g32.double() - g64).abs().max())
        tol = mult * max(MARGIN * e32 / scale, FLOOR)
        print(f"{tag} grad {j}: err {e / scale:.2e} max|g64| (f32 torch {e32 / scale:.2e}, bound {tol:.2e})")
        assert e / scale <= tol, (tag, j, e / scale, tol)
        _note(op, 1, e32 / scale), _note(op, 3, e / scale)


def _backward(vals):
    tot = sum(c * v.sum() for c, v in zip(COEF, vals) if v is not None)
    if torch.is_tensor(tot) and tot.requires_grad:
        tot.backward()


def _ref_run(fn, inputs):
    """fn(dtype, *leaves) -> tuple of tensors (None entries dropped); -> ((values, grads) float32, (values, grads) float64)"""
    out = []
    for dtype in (torch.float32, torch.float64):
        ls = [leaf(x, dtype=dtype) for x in inputs]
        vals = fn(dtype, *ls)
        _backward(vals)
        out.append(([v.detach() for v in vals if v is not None], [x.grad if x.grad is not None else torch.zeros_like(x) for x in ls]))
    return out


def _op_run(fn, inputs, backend):
    ls = [leaf(x, backend) for x in inputs]
    vals = fn(*ls)
    _backward(vals)
    sync(backend)
    return [v for v in vals if v is not None], [x.grad if x.grad is not None else torch.zeros_like(x) for x in ls]


def _count(monkeypatch, fn):
    monkeypatch.setattr(_lib, "CALL_COUNT", 0)
    out = fn()
    n = _lib.CALL_COUNT
    monkeypatch.setattr(_lib, "CALL_COUNT", None)
    return out, n


# ------------------------------------------------------------------------------------------------ 1. remain mask
FAR, THRESH = 5.0, 0.75          # 5, 0.8 * 5 = 4 and 0.75 are exact in float32: a value ON them is decided by the strict >


def _mask_inputs(H, W, seed, on_thresholds=False):
    g = torch.Generator().manual_seed(seed)
    n = H * W
    mp = torch.rand(n, generator=g)
    mp = torch.where((mp - THRESH).abs() < 1e-3, mp + 0.01, mp)
    d0 = torch.rand(n, generator=g) * 8.0
    d1 = torch.rand(n, generator=g) * 8.0
    dg = torch.rand(n, generator=g) * 3.0 + 0.1
    for d in (d0, d1):
        for thr in (FAR, 0.8 * FAR):
            d[((d - thr).abs() < 2e-3 * thr)] += 0.05
    mean = float(dg.double().mean())
    dg[(dg - mean).abs() < 2e-3 * mean] += 0.05
    mean = float(dg.double().mean())
    if on_thresholds:
        k = min(n, 3)
        mp[:k] = torch.tensor([THRESH, THRESH + 2.0 ** -20, THRESH - 2.0 ** -20])[:k]
        d0[:k] = torch.tensor([FAR, FAR + 2.0 ** -20, FAR - 2.0 ** -20])[:k]
        d1[:k] = torch.tensor([0.8 * FAR, 0.8 * FAR + 2.0 ** -20, 0.8 * FAR - 2.0 ** -20])[:k]
    else:
        assert float((mp - THRESH).abs().min()) >= 1e-3
        for d in (d0, d1):
            assert float(((d - FAR).abs() / FAR).min()) >= 1e-3 and float(((d - 0.8 * FAR).abs() / (0.8 * FAR)).min()) >= 1e-3
        # (one pixel IS its mean: it sits 1e-5 = 80 float32 ulps above the gate mean - 1e-5, whatever the summation order)
        assert n == 1 or float(((dg - mean).abs() / mean).min()) >= 1e-3
    occ, dyn, hum = (torch.rand(n, generator=g) > 0.2), (torch.rand(n, generator=g) > 0.85), (torch.rand(n, generator=g) > 0.9)
    sh = (H, W)
    return dict(mask_pred=mp.view(sh), depth_pred0=d0.view(sh), depth_pred=d1.view(sh), depth_gt=dg.view(sh), occupancy_gt=occ.view(sh),
                dynamic_gt=dyn.view(sh), human_gt=hum.view(sh))


def _mask_op(maps, backend, **kw):
    out = losses.mono_remain_mask(**{k: v.to(backend) for k, v in maps.items()}, far=FAR, mask_pred_thresh=THRESH, **kw)
    sync(backend)
    assert out.dtype == torch.bool and not out.requires_grad
    return out.cpu()


def test_erosion_reference_forms_agree():
    """the pooled form the cases use equals the explicit window loop, also for 2e larger than the image"""
    g = torch.Generator().manual_seed(3)
    for H, W in [(1, 1), (1, 7), (5, 9), (17, 33)]:
        m = torch.rand(H, W, generator=g) > 0.15
        for e in (1, 2, 8):
            assert torch.equal(ref.erode(m, e), ref.erode_fast(m, e)), (H, W, e)
    m = torch.ones(5, 5, dtype=torch.bool)
    m[2, 2] = False
    want = torch.ones(5, 5, dtype=torch.bool)
    want[2:4, 2:4] = False                  # rows y-1 .. y, columns x-1 .. x contain (2, 2) for y, x in {2, 3}
    assert torch.equal(ref.erode(m, 1), want)


@pytest.mark.parametrize("H,W", SHAPES)
def test_remain_mask_exact(backend, H, W):
    maps = _mask_inputs(H, W, 11 + H * W)
    lists = [[n] for n in ref.IGNORE] + [list(ref.IGNORE), []]
    for names in lists:
        for e in (0, 1, 2, 8):
            for for_normals in (False, True):
                kw = dict(ignore_mask_list=names, mask_erode=e, for_normals=for_normals)
                want = ref.remain_mask(**maps, far=FAR, mask_pred_thresh=THRESH, fast=True, **kw)
                got = _mask_op(maps, backend, **kw)
                assert torch.equal(got, want), (names, e, for_normals, int((got != want).sum()))
    # the two quirks: the depth loss with an empty list keeps everything, the normal loss still builds (and erodes) its mask
    assert bool(_mask_op(maps, backend, ignore_mask_list=[], mask_erode=2).all())
    flat = {k: v.reshape(-1) for k, v in maps.items()}
    assert torch.equal(_mask_op(flat, backend, ignore_mask_list=list(ref.IGNORE)),
                       ref.remain_mask(**maps, far=FAR, mask_pred_thresh=THRESH, ignore_mask_list=list(ref.IGNORE)).reshape(-1))


def test_remain_mask_on_the_thresholds(backend):
    """values ON each threshold stay (strict >), one ulp-ish above goes"""
    maps = _mask_inputs(5, 9, 5, on_thresholds=True)
    for names, key in ((["pred_not_occupied"], None), (["toofar"], None), (["pred_distant"], None)):
        got = _mask_op(maps, backend, ignore_mask_list=names).reshape(-1)
        want = ref.remain_mask(**maps, far=FAR, mask_pred_thresh=THRESH, ignore_mask_list=names).reshape(-1)
        assert torch.equal(got, want)
        if names == ["pred_not_occupied"]:
            assert got[:3].tolist() == [False, True, False]        # mask_pred == thresh is NOT occupied
        else:
            assert got[:3].tolist() == [True, False, True]         # depth == far is not too far
    # mono_distant: a prior of two exactly representable levels, mean 1.5: 2 > 1.5 - 1e-5 goes, 1 stays
    dg = torch.tensor([1.0, 2.0]).repeat(3).view(2, 3)
    got = losses.mono_remain_mask(depth_gt=dg.to(backend), ignore_mask_list=["mono_distant"]).cpu()
    assert torch.equal(got, dg < 1.5)


def test_remain_mask_refusals(backend):
    maps = {k: v.to(backend) for k, v in _mask_inputs(4, 4, 1).items()}
    with pytest.raises(ValueError, match="human_gt"):
        losses.mono_remain_mask(maps["mask_pred"], ignore_mask_list=["human"])
    with pytest.raises(ValueError, match="unknown ignore_mask_list entry 'cars'"):
        losses.mono_remain_mask(maps["mask_pred"], ignore_mask_list=["cars"])
    with pytest.raises(ValueError, match="need far"):
        losses.mono_remain_mask(maps["mask_pred"], depth_pred0=maps["depth_pred0"], ignore_mask_list=["toofar"])
    with pytest.raises(ValueError, match="2-D"):
        losses.mono_remain_mask(maps["mask_pred"].reshape(-1), ignore_mask_list=["pred_not_occupied"], mask_erode=1)
    with pytest.raises(NotImplementedError, match="mask_erode=33"):
        losses.mono_remain_mask(maps["mask_pred"], ignore_mask_list=["pred_not_occupied"], mask_erode=33)
    with pytest.raises(TypeError):
        losses.mono_remain_mask(maps["mask_pred"], erode=1)


# ------------------------------------------------------------------------------------------------ 2. scale-and-shift-invariant depth
MASKS = ("ones", "random", "one", "empty")
SSI_OPTS = [(sg, dt, sc, pre, mk) for sg in (False, True) for dt in (False, True) for sc in (0, 1, 4) for pre in ((1.0, 0.0), (50.0, 1.0))
            for mk in MASKS]


def _rotation(i):
    """eight combinations in which every value of every option occurs; ``i`` rotates them from fn_type to fn_type"""
    out = []
    for k in range(8):
        j = k + i
        out.append(((k & 1) == 1, (k >> 1 & 1) == 1, (0, 1, 4)[j % 3], ((1.0, 0.0), (50.0, 1.0))[(k >> 2) & 1], MASKS[j % 4]))
    return out


def _depth_inputs(H, W, seed, kind):
    g = torch.Generator().manual_seed(seed)
    pred = torch.rand(H, W, generator=g) * 5.0 + 0.5
    gt = 0.3 * pred + 0.1 + 0.05 * torch.randn(H, W, generator=g)
    n = H * W
    if kind == "ones":
        mask = torch.ones(H, W, dtype=torch.bool)
    elif kind == "random":
        mask = torch.rand(H, W, generator=g) < 0.6
        mask.view(-1)[:min(n, 3)] = True          # (an exact fit of two points leaves residuals of rounding noise: |0| has no gradient)
    elif kind == "one":
        mask = torch.zeros(H, W, dtype=torch.bool)
        mask.view(-1)[n // 2] = True
    else:
        mask = torch.zeros(H, W, dtype=torch.bool)
    return pred, gt, mask


def _ssi_case(backend, H, W, fn_type, opt, seed):
    sg, dt, sc, pre, mk = opt
    pred, gt, mask = _depth_inputs(H, W, seed, mk)
    aux = {}
    ref.ssi_depth(pred.double(), gt, mask, torch.float64, gt_pre_scale=pre[0], gt_pre_shift=pre[1], aux=aux)
    if sg and float(aux["det"]) == 0.0:
        return False                            # the reference divides by zero there
    kw = dict(fn_type=fn_type, gt_pre_scale=pre[0], gt_pre_shift=pre[1], scale_gt_to_pred=sg, detach_scale_shift=dt,
              alpha_grad_reg=0.0 if sc == 0 else 0.01, grad_reg_scales=4 if sc == 0 else sc, w=0.7)
    r32, r64 = _ref_run(lambda d, p: ref.ssi_depth(p, gt, mask, d, **kw), [pred])
    vals, grads = _op_run(lambda p: losses.mono_depth_ssi_loss(p, gt.to(backend), mask.to(backend), **kw), [pred], backend)
    tag = f"ssi {H}x{W} {fn_type} sgp={sg} detach={dt} scales={sc} pre={pre} mask={mk}"
    assert len(vals) == (1 if sc == 0 else 2), tag
    _check("ssi depth", tag, vals, grads, r32, r64)
    if mk == "empty" or (mk == "one" and not sg):
        if mk == "empty":
            assert all(float(v.detach()) == 0.0 for v in vals), tag
        assert float(grads[0].abs().max()) == 0.0, tag          # det == 0: scale = shift = 0, nothing reaches pred
    return True


@pytest.mark.parametrize("fn_type", ref.FN_TYPES)
@pytest.mark.parametrize("H,W", SHAPES)
def test_ssi_depth_matches_float64(backend, H, W, fn_type):
    opts = SSI_OPTS if (H, W) in SMALL else _rotation(ref.FN_TYPES.index(fn_type))
    ran = sum(_ssi_case(backend, H, W, fn_type, opt, 1000 + 7 * i + H * W) for i, opt in enumerate(opts))
    assert ran >= len(opts) // 2


def test_ssi_gradient_goes_through_the_solve(backend):
    """5x9, l1 and the regulariser: against torch.autograd through the float64 restatement, which differentiates through the solve;
    the part of the gradient that comes through (scale, shift) is far above the bound, so dropping it cannot pass"""
    H, W = 5, 9
    pred, gt, mask = _depth_inputs(H, W, 77, "random")
    kw = dict(fn_type="l1", alpha_grad_reg=0.01, grad_reg_scales=4, w=1.0)
    r32, r64 = _ref_run(lambda d, p: ref.ssi_depth(p, gt, mask, d, **kw), [pred])
    _, rd = _ref_run(lambda d, p: ref.ssi_depth(p, gt, mask, d, detach_scale_shift=True, **kw), [pred])
    chain = float((r64[1][0] - rd[1][0]).abs().max() / r64[1][0].abs().max())
    print(f"chain term: {chain:.3e} of max |g64|")
    assert chain > 1e-2
    vals, grads = _op_run(lambda p: losses.mono_depth_ssi_loss(p, gt.to(backend), mask.to(backend), **kw), [pred], backend)
    _check("ssi depth", "ssi chain", vals, grads, r32, r64)
    vals_d, grads_d = _op_run(lambda p: losses.mono_depth_ssi_loss(p, gt.to(backend), mask.to(backend), detach_scale_shift=True, **kw),
                              [pred], backend)
    assert float((grads_d[0].cpu().double() - rd[1][0]).abs().max() / rd[1][0].abs().max()) < 1e-5
    assert float(vals_d[0]) == float(vals[0])


def test_ssi_refusals(backend):
    p, g = torch.rand(4, 5, device=backend), torch.rand(4, 5, device=backend)
    m = torch.ones(4, 5, dtype=torch.bool, device=backend)
    with pytest.raises(NotImplementedError, match="fn_type='l3'"):
        losses.mono_depth_ssi_loss(p, g, m, fn_type="l3")
    with pytest.raises(TypeError, match="'delta'"):
        losses.mono_depth_ssi_loss(p, g, m, fn_type="huber", fn_param=dict(delta=1.0))
    with pytest.raises(NotImplementedError, match="gt.requires_grad"):
        losses.mono_depth_ssi_loss(p, g.clone().requires_grad_(True), m)
    with pytest.raises(ValueError, match=r"\[H,W\]"):
        losses.mono_depth_ssi_loss(p.reshape(-1), g.reshape(-1), m.reshape(-1))
    with pytest.raises(TypeError, match="bool or uint8"):
        losses.mono_depth_ssi_loss(p, g, m.float())
    with pytest.raises(TypeError):
        losses.mono_depth_ssi_loss(p, g, m, reduction="mean")
    d, r = losses.mono_depth_ssi_loss(p, g, m, alpha_grad_reg=0.0)
    assert r is None and d.shape == ()
    d2, _ = losses.mono_depth_ssi_loss(p.t().contiguous().t(), g, m, fn_param={})          # a non-contiguous prediction
    assert float(d2) == float(d)


# ------------------------------------------------------------------------------------------------ 3. Pearson depth
@pytest.mark.parametrize("H,W", SHAPES)
def test_pearson_depth_matches_float64(backend, H, W):
    for i, (sc, mk) in enumerate([(4, "ones"), (4, "random"), (1, "random"), (0, "random"), (4, "one"), (4, "empty")]):
        pred, gt, mask = _depth_inputs(H, W, 300 + i + H * W, mk)
        if mk in ("ones", "random") and int(mask.sum()) >= 2:
            assert float(pred[mask].var()) > 1e-4 and float(gt[mask].var()) > 1e-6        # non-zero variance in every masked set
        kw = dict(alpha_grad_reg=0.0 if sc == 0 else 0.01, grad_reg_scales=4 if sc == 0 else sc, w=0.7)
        r32, r64 = _ref_run(lambda d, p: ref.pearson_depth(p, gt, mask, d, **kw), [pred])
        vals, grads = _op_run(lambda p: losses.mono_depth_pearson_loss(p, gt.to(backend), mask.to(backend), **kw), [pred], backend)
        assert len(vals) == (1 if sc == 0 else 2)
        _check("pearson depth", f"pearson {H}x{W} scales={sc} mask={mk}", vals, grads, r32, r64, unit=0.7 * 0.01)
        if mk == "empty":
            assert all(float(v) == 0.0 for v in vals) and float(grads[0].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 4. normal cue
def _rotations(n, g):
    q = torch.randn(n, 4, generator=g)
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                        2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).view(n, 3, 3)


@pytest.mark.parametrize("rot_kind", ["none", "one", "per_row"])
@pytest.mark.parametrize("N", NS)
def test_normal_cue_matches_float64(backend, N, rot_kind):
    g = torch.Generator().manual_seed(40 + N)
    npred, ngt = torch.randn(N, 3, generator=g) * 1.7, torch.randn(N, 3, generator=g)
    mask = torch.rand(N, generator=g) < 0.7
    rot = None if rot_kind == "none" else (_rotations(1, g)[0] if rot_kind == "one" else _rotations(N, g))
    if N >= 63:
        npred[5] = 0.0                     # a zero predicted normal under a cleared mask: a finite, zero gradient
        mask[5] = False
        mask[7] = True                     # pred == gt (after the rotation: identity rows only): sign(0) = 0
        if rot_kind == "none":
            npred[7] = ngt[7] = torch.tensor([0.0, 0.6, -0.8])
        elif rot_kind == "per_row":
            rot[7] = torch.eye(3)
            npred[7] = ngt[7] = torch.tensor([0.0, 0.6, -0.8])
    for m in (mask, None):
        kw = dict(w_l1=0.03, w_cos=0.02)
        r32, r64 = _ref_run(lambda d, p: ref.normal_cue(p, ngt, m, d, rot=rot, **kw), [npred])
        vals, grads = _op_run(lambda p: losses.mono_normal_cue_loss(p, ngt.to(backend), None if m is None else m.to(backend),
                                                                    rot=None if rot is None else rot.to(backend), **kw), [npred], backend)
        _check("normal cue", f"normals N={N} rot={rot_kind} mask={m is not None}", vals, grads, r32, r64)
        if m is not None:
            assert torch.equal(grads[0].cpu()[~mask], torch.zeros(int((~mask).sum()), 3))


def test_normal_cue_refusals(backend):
    a, b = torch.randn(6, 3, device=backend), torch.randn(6, 3, device=backend)
    with pytest.raises(ValueError, match="rot must be"):
        losses.mono_normal_cue_loss(a, b, rot=torch.eye(3, device=backend).repeat(5, 1, 1))
    with pytest.raises(NotImplementedError, match="normals_gt.requires_grad"):
        losses.mono_normal_cue_loss(a, b.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="rows of the normals"):
        losses.mono_normal_cue_loss(a, b, torch.ones(5, dtype=torch.bool, device=backend))
    with pytest.raises(TypeError):
        losses.mono_normal_cue_loss(a, b, w_sin=1.0)


# ------------------------------------------------------------------------------------------------ 5. an object's share
def _share_buffer(N, seed):
    """packs of length 0, 1, 64, 65 and 300 among random ones; every fourth ray not hit"""
    g = torch.Generator().manual_seed(seed)
    hit = torch.tensor([i for i in range(N) if N < 3 or i % 4 != 1], dtype=torch.long)
    n = torch.randint(2, 13, [hit.shape[0]], generator=g)
    for k, v in enumerate((0, 1, 64, 65, 300)):
        if hit.shape[0] > 2 * k:
            n[2 * k] = v
    pi = torch.stack([torch.cumsum(n, 0) - n, n], dim=1)
    S = int(n.sum())
    vw = torch.rand(S, generator=g) * 0.05
    return dict(hit=hit, pi=pi, vw=vw, t=torch.rand(S, generator=g) * 6 + 0.2, rgb=torch.rand(S, 3, generator=g),
                nab=torch.randn(S, 3, generator=g) * 1.2)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("norm_depth,norm_nab,with_rgb,with_nab", [(True, False, True, True), (False, True, True, True),
                                                                  (True, True, False, True), (False, False, True, False),
                                                                  (True, False, False, False)])
def test_packed_share_matches_float64(backend, N, norm_depth, norm_nab, with_rgb, with_nab):
    b = _share_buffer(N, 60 + N)
    if int(b["vw"].numel()) == 0:
        b["vw"], b["t"], b["rgb"], b["nab"] = torch.rand(0), torch.rand(0), torch.rand(0, 3), torch.rand(0, 3)
    inputs = [b["vw"]] + ([b["rgb"]] if with_rgb else []) + ([b["nab"]] if with_nab else [])

    def split(ls):
        ls = list(ls)
        return ls[0], (ls[1] if with_rgb else None), (ls[-1] if with_nab else None)

    def fn_ref(d, *ls):
        vw, rgb, nab = split(ls)
        o = ref.share(vw, b["t"], rgb, nab, b["pi"], b["hit"], N, d, norm_depth, norm_nab)
        return [o["mask_volume"], o["depth_volume"], o.get("rgb_volume"), o.get("normals_volume")]

    def fn_op(*ls):
        vw, rgb, nab = split(ls)
        return list(losses.packed_share(vw, b["t"].to(backend), rgb, nab, b["pi"].to(backend), b["hit"].to(backend), N, norm_depth, norm_nab))
    r32, r64 = _ref_run(fn_ref, inputs)
    vals, grads = _op_run(fn_op, inputs, backend)
    _check("packed share", f"share N={N} nd={norm_depth} nn={norm_nab} rgb={with_rgb} nab={with_nab}", vals, grads, r32, r64)
    miss = torch.ones(N, dtype=torch.bool)
    miss[b["hit"]] = False
    for v in vals:
        assert float(v.detach().cpu()[miss].abs().sum()) == 0.0          # rays the object does not hit: zeros


def test_rendered_share_of_an_empty_buffer(backend):
    out = losses.rendered_share(dict(type="empty"), 7, device=backend, with_rgb=True, with_normal=True)
    assert sorted(out) == ["depth_volume", "mask_volume", "normals_volume", "rgb_volume"]
    assert all(float(v.abs().sum()) == 0.0 for v in out.values()) and out["rgb_volume"].shape == (7, 3)


# ------------------------------------------------------------------------------------------------ 6. launch budget
def test_launch_budget(backend, monkeypatch):
    """C-ABI calls per direction: mask 1 (2 with mono_distant), SSI <= 2 + 1, Pearson <= 2 + 1, normals 1 + 1, share 1 + 1 -- at 80x120,
    a multi-workgroup grid"""
    H, W = 80, 120
    maps = {k: v.to(backend) for k, v in _mask_inputs(H, W, 9).items()}
    _, n = _count(monkeypatch, lambda: losses.mono_remain_mask(**maps, far=FAR, ignore_mask_list=["toofar", "human", "pred_not_occupied"],
                                                               mask_erode=8))
    assert n == 1
    _, n = _count(monkeypatch, lambda: losses.mono_remain_mask(**maps, far=FAR, ignore_mask_list=list(ref.IGNORE), mask_erode=8))
    assert n == 2
    pred, gt, mask = _depth_inputs(H, W, 10, "random")
    b = _share_buffer(64, 12)
    g = torch.Generator().manual_seed(13)
    cases = {
        "ssi": (2, lambda p: sum(losses.mono_depth_ssi_loss(p, gt.to(backend), mask.to(backend), fn_type="l1")), [pred]),
        "pearson": (2, lambda p: sum(losses.mono_depth_pearson_loss(p, gt.to(backend), mask.to(backend))), [pred]),
        "normals": (1, lambda p: sum(losses.mono_normal_cue_loss(p, torch.randn(300, 3, generator=g).to(backend),
                                                                 rot=_rotations(300, g).to(backend))), [torch.randn(300, 3, generator=g)]),
        "share": (1, lambda vw, rgb: sum(v.sum() for v in losses.packed_share(vw, b["t"].to(backend), rgb, None, b["pi"].to(backend),
                                                                            b["hit"].to(backend), 64) if v is not None), [b["vw"], b["rgb"]]),
    }
    for name, (fwd_max, fn, inputs) in cases.items():
        ls = [leaf(t, backend) for t in inputs]
        loss, n_fwd = _count(monkeypatch, lambda: fn(*ls))
        _, n_bwd = _count(monkeypatch, loss.backward)
        sync(backend)
        print(f"{name}: {n_fwd} C-ABI calls forward, {n_bwd} backward")
        assert 1 <= n_fwd <= fwd_max and n_bwd == 1, (name, n_fwd, n_bwd)
        assert all(t.grad is not None and float(t.grad.abs().max()) > 0 for t in ls)


# ------------------------------------------------------------------------------------------------ 7. renderer
def _street(backend, loss_cfg=None, **kw):
    from neuralsim_amd import scenarios as sc
    torch.manual_seed(1234)
    return sc.build_street_trainer(backend, small=True, rays_per_gpu=48, num_uniform=16, loss_cfg=loss_cfg, **kw)


def test_renderer_shares_add_up_to_the_joint_rendering(backend):
    """small street models with the distant model: main + distant == the joint rendering in mask, rgb before the sky blend and
    un-normalised depth; every share equals the restatement on the object's own buffer; the flags left off change no key"""
    tr = _street(backend)
    tr.renderer.config.update(depth_use_normalized_vw=False)
    xy, fidx, _ = tr.sample_batch()
    state = tr.gen.get_state()
    base = tr.render(xy, fidx)
    assert sorted(base) == ["raw_per_obj_model", "ray_intersections", "rays_d", "rays_o", "rendered", "volume_buffer"]   # today's keys
    tr.gen.set_state(state)
    tr._mono_per_obj = True
    ret = tr.render(xy, fidx)
    sync(backend)
    assert sorted(set(ret) - set(base)) == ["rendered_per_obj_in_scene"]
    per = ret["rendered_per_obj_in_scene"]
    assert sorted(per) == ["distant", "main"]
    N, tot = xy.shape[0], ret["rendered"]
    raw = ret["raw_per_obj_model"]
    assert raw["main"]["volume_buffer"]["type"] != "empty"
    for key, tkey in (("mask_volume", "mask_volume"), ("depth_volume", "depth_volume"), ("rgb_volume", "rgb_volume_occupied"),
                      ("normals_volume", "normals_volume")):
        r = {}
        for dt in (torch.float32, torch.float64):
            parts = []
            for oid in ("main", "distant"):
                vb = raw[oid]["volume_buffer"]
                c = lambda t_: t_.detach().cpu().to(dt)          # noqa: E731
                nab = c(vb["nablas_in_world"]).flatten(0, -2) if "nablas_in_world" in vb else None
                parts.append(ref.share(c(vb["vw_in_total"]).reshape(-1), c(vb["t"]).reshape(-1), c(vb["rgb"]).flatten(0, -2), nab,
                                       vb["pack_infos_collect"].cpu(), vb["rays_inds_collect"].cpu(), N, dt, normalized_depth=False))
            r[dt] = parts
        zero = torch.zeros(N, 3, dtype=torch.float64)
        for oid, p32, p64 in zip(("main", "distant"), r[torch.float32], r[torch.float64]):
            _check("packed share", f"renderer {oid} {key}", [per[oid][key]], [], ([p32.get(key, zero.float())], []), ([p64.get(key, zero)], []))
        s64 = sum(p.get(key, zero) for p in r[torch.float64])
        s32 = sum(p.get(key, zero.float()) for p in r[torch.float32])
        scale, e32 = float(s64.abs().max()), float((s32.double() - s64).abs().max())
        e = float(((per["main"][key] + per["distant"][key]).detach().cpu().double() - tot[tkey].detach().cpu().double()).abs().max())
        tol = max(MARGIN * e32, FLOOR * scale)
        print(f"renderer main + distant vs joint {key}: err {e:.2e} (f32 torch {e32:.2e}, bound {tol:.2e}, scale {scale:.2e})")
        assert e <= tol, (key, e, tol)
    # per class: the main class, Distant, and the sky's blend with the residual transmittance
    tr.gen.set_state(state)
    rays_o, rays_d = ret["rays_o"], ret["rays_d"]
    from neuralsim_amd.losses import embedding_lookup
    ret2 = tr.renderer.render(tr.model, rays=[rays_o, rays_d], rays_h_appear=embedding_lookup(tr.appear, fidx), with_normal=True,
                              distant_model=tr.distant_model, sky_model=tr.sky_model, render_per_class_in_scene=True)
    sync(backend)
    pc = ret2["rendered_per_class_in_scene"]
    assert sorted(pc) == ["Distant", "Main", "Sky"] and "rendered_per_obj_in_scene" not in ret2
    assert torch.equal(pc["Sky"]["rgb_volume"], ret2["rendered"]["rgb_volume_non_occupied"])


# ------------------------------------------------------------------------------------------------ 8. trainer
REPLICA_DEPTH = dict(fn_type="mse", w=1.0e-3, w_grad_reg=1.0e-5, gt_pre_scale=50.0, gt_pre_shift=1.0, ignore_mask_list=[],
                     mask_pred_thresh=0.5, mask_erode=8, enable_after=1500, detach_scale_shift=False, scale_gt_to_pred=False)
REPLICA_NORMALS = dict(w_l1=0.01, w_cos=0.01, ignore_mask_list=[], apply_in_pixel_train_step=True)
STREET_DEPTH = dict(w=1.0e-4, fn_type="l2", w_grad_reg=1.0e-6, distant_mode="cr_only", gt_pre_scale=80.0, gt_pre_shift=1.0,
                    ignore_mask_list=["pred_not_occupied", "human", "not_occupied"], mask_pred_thresh=0.5, mask_erode=8, grad_reg_scales=4,
                    enable_after=1000, detach_scale_shift=False, scale_gt_to_pred=False)
STREET_NORMALS = dict(distant_mode="cr_only", w_l1=0.01, w_cos=0.01, ignore_mask_list=["pred_not_occupied", "human"],
                      mask_pred_thresh=0.95, apply_in_pixel_train_step=True)


def test_flat_yaml_keys_map_onto_the_constructor_arguments():
    """the two yaml blocks (lotd_neus.replica.230814.yaml:271-288, withmask_nolidar.240219.yaml:463-483) as literals"""
    from neuralsim_amd import scenarios as sc
    assert sc.INDOOR_MONO_LOSS_CFG == dict(mono_depth=REPLICA_DEPTH, mono_normals=REPLICA_NORMALS)
    d = losses.mono_depth_cfg(REPLICA_DEPTH)
    assert d == dict(w=1.0e-3, anneal=None, loss_type="monosdf", far=None, distant_mode=None, ignore_mask_list=[], mask_pred_thresh=0.5,
                     mask_erode=8, enable_after=1500,
                     loss_param=dict(fn_type="mse", gt_pre_scale=50.0, gt_pre_shift=1.0, detach_scale_shift=False, scale_gt_to_pred=False,
                                     alpha_grad_reg=1.0e-5 / 1.0e-3))
    s = losses.mono_depth_cfg(STREET_DEPTH)
    assert s["loss_type"] == "monosdf" and s["distant_mode"] == "cr_only" and s["mask_erode"] == 8 and s["enable_after"] == 1000
    assert s["loss_param"] == dict(fn_type="l2", gt_pre_scale=80.0, gt_pre_shift=1.0, grad_reg_scales=4, detach_scale_shift=False,
                                   scale_gt_to_pred=False, alpha_grad_reg=1.0e-6 / 1.0e-4)
    assert losses.mono_depth_cfg({})["loss_type"] == "pearson"              # the class default (mono.py:257)
    n = losses.mono_normals_cfg(STREET_NORMALS)
    assert n == dict(w_l1=0.01, w_cos=0.01, loss_per="pixels", distant_mode="cr_only", ignore_mask_list=["pred_not_occupied", "human"],
                     mask_pred_thresh=0.95, mask_erode=0, apply_in_pixel_train_step=True, enable_after=0)
    assert losses.mono_normals_cfg(REPLICA_NORMALS)["ignore_mask_list"] == []
    with pytest.raises(TypeError, match="'w_reg'"):
        losses.mono_depth_cfg(dict(REPLICA_DEPTH, w_reg=1.0))
    with pytest.raises(TypeError, match="'fn_type'"):
        losses.mono_depth_cfg(dict(loss_type="pearson", fn_type="l1"))
    with pytest.raises(TypeError, match="'beta'"):
        losses.mono_depth_cfg(dict(loss_type="pearson", loss_param=dict(beta=1.0)))
    with pytest.raises(NotImplementedError, match="points"):
        losses.mono_normals_cfg(dict(loss_per="points"))


def _indoor(backend, loss_cfg, **kw):
    from neuralsim_amd import scenarios as sc
    torch.manual_seed(1234)
    return sc.build_indoor_trainer(backend, small=True, rays_per_gpu=96, num_uniform=16, loss_cfg=loss_cfg, **kw)


def test_trainer_indoor_blocks(backend, monkeypatch):
    """the replica yaml's two blocks on the small indoor trainer (an 8x8 patch): the terms under the reference's keys, equal to the
    restatement on the same render, three finite steps"""
    from neuralsim_amd import scenarios as sc
    tr = _indoor(backend, sc.INDOOR_MONO_LOSS_CFG)
    seen = {}
    loss = tr.loss

    def spy(ret, gt, uni=None, aux=None):
        seen.update(ret=ret, aux=aux)
        return loss(ret, gt, uni, aux=aux)
    monkeypatch.setattr(tr, "loss", spy)
    first = float(tr.train_step(0))
    # before ``enable_after: 1500`` the depth block is off (and the plain-torch depth term stays replaced); the normals are on
    assert sorted(tr.loss_parts) == ["loss_eikonal", "loss_mono_normal.cos", "loss_mono_normal.l1", "loss_rgb"]
    ls = [first] + [float(tr.train_step(it)) for it in (1500, 1501)]
    sync(backend)
    assert all(math.isfinite(l) for l in ls)
    keys = ["loss_eikonal", "loss_mono_depth.depth", "loss_mono_depth.reg", "loss_mono_normal.cos", "loss_mono_normal.l1", "loss_rgb"]
    assert sorted(tr.loss_parts) == keys
    r, aux = seen["ret"]["rendered"], seen["aux"]
    ph, pw = tr.mono["patch_hw"]
    P = ph * pw
    c = lambda t_: t_.detach().cpu()          # noqa: E731
    mv, dv, nv = c(r["mask_volume"]), c(r["depth_volume"]), c(r["normals_volume"])
    remain = ref.remain_mask(mv[:P].view(ph, pw), ignore_mask_list=[], mask_pred_thresh=0.5, mask_erode=8)
    assert bool(remain.all())                 # the depth loss with an empty list keeps every pixel, erosion or not
    kw = dict(fn_type="mse", gt_pre_scale=50.0, gt_pre_shift=1.0, alpha_grad_reg=1.0e-2, grad_reg_scales=4, w=1.0e-3)
    gt = c(aux["depth"])[:P].view(ph, pw)
    r32, r64 = _ref_run(lambda d_, p: ref.ssi_depth(p, gt, remain, d_, **kw), [dv[:P].view(ph, pw)])
    parts = tr.loss_parts
    _check("ssi depth", "trainer depth", [parts["loss_mono_depth.depth"], parts["loss_mono_depth.reg"]], [], (r32[0], []), (r64[0], []))
    ones = torch.ones(mv.shape[0], dtype=torch.bool)
    n32, n64 = _ref_run(lambda d_, p: ref.normal_cue(p, c(aux["normals"]), ones, d_, w_l1=0.01, w_cos=0.01), [nv])
    _check("normal cue", "trainer normals", [parts["loss_mono_normal.l1"], parts["loss_mono_normal.cos"]], [], (n32[0], []), (n64[0], []))


def test_trainer_without_mono_blocks_is_bit_identical(backend):
    """an indoor trainer built by the parent's signature and one handed ``loss_cfg=None``: the same path (the plain-torch mono terms),
    the same losses and parameters over three iterations -- exactly on the emulator, within the allowance
    ``test_trainer_without_loss_cfg_is_bit_identical`` of tests/test_street_losses.py gives two runs on the device"""
    outs = []
    for kw in (dict(), dict(loss_cfg=None)):
        from neuralsim_amd import scenarios as sc
        torch.manual_seed(1234)
        tr = sc.build_indoor_trainer(backend, small=True, rays_per_gpu=96, num_uniform=16, **kw)
        assert tr.loss_cfg is None and tr._mono_per_obj is False
        ls = [float(tr.train_step(it)) for it in range(3)]
        sync(backend)
        assert sorted(tr.loss_parts) == ["loss_eikonal", "loss_rgb"]
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
        assert float(bad.float().mean()) < 2e-3 and float(d.max()) <= 2 * 3 * 1e-3      # 3 iterations x lr


def _street_mono(backend, depth=None, normals=None, **mono_kw):
    """a small street trainer with synthetic priors: the analytic world's depth / normal images and a fake human mask"""
    from neuralsim_amd import scenarios as sc
    from neuralsim_amd.trainer import RenderTrainer
    torch.manual_seed(1234)
    world = sc.street_world()
    m, dm, sm = sc.street_models(backend, "fp16", 42, True, world)
    m.accel.init(m.query_sdf, generator=torch.Generator(device=backend).manual_seed(42))
    intr, c2w, WH = sc.street_rig(n_ego=2, H=24, W=24, f=15.0, device=backend)
    img, dep, nrm = sc.render_dataset(world, intr, c2w, WH, with_mono=True)
    human = torch.zeros(dep.shape, dtype=torch.bool, device=backend)
    human[:, 10:14, 8:12] = True
    cfg = {k: v for k, v in (("mono_depth", depth), ("mono_normals", normals)) if v is not None}
    mono = dict(depth=dep, normals=nrm, patch_hw=(6, 7), human_mask=human, **mono_kw)
    return RenderTrainer(m, intr, c2w, WH, num_rays=64, lr=1e-3, w_eikonal=0.01, num_uniform=16, near=0.1, far=200.0, seed=42,
                         learn_inv_s=False, distant_model=dm, sky_model=sm, target_images=img, rgb_fn="l1", loss_cfg=cfg or None,
                         target_masks=sc.render_occupancy_masks(world, intr, c2w, WH), mono=mono)


def test_trainer_street_cr_only_uses_the_per_object_rendering(backend, monkeypatch):
    """the street yaml's blocks (``distant_mode: cr_only``, human / occupancy masks, a 6x7 patch with mask_erode 1): the depth term
    is taken on ``rendered_per_obj_in_scene['main']``, and equals the restatement there"""
    tr = _street_mono(backend, dict(STREET_DEPTH, enable_after=0, mask_erode=1), STREET_NORMALS, normals_in_camera_frame=True)
    assert tr._mono_per_obj
    seen = {}
    loss = tr.loss

    def spy(ret, gt, uni=None, aux=None):
        seen.update(ret=ret, aux=aux)
        return loss(ret, gt, uni, aux=aux)
    monkeypatch.setattr(tr, "loss", spy)
    ls = [float(tr.train_step(it)) for it in range(2)]
    sync(backend)
    assert all(math.isfinite(l) for l in ls)
    ret, aux, parts = seen["ret"], seen["aux"], tr.loss_parts
    assert sorted(ret["rendered_per_obj_in_scene"]) == ["distant", "main"]
    ph, pw = 6, 7
    P = ph * pw
    c = lambda t_: t_.detach().cpu()          # noqa: E731
    main, r = ret["rendered_per_obj_in_scene"]["main"], ret["rendered"]
    sh = (ph, pw)
    remain = ref.remain_mask(c(main["mask_volume"])[:P].view(sh), occupancy_gt=c(aux["mask"])[:P].view(sh) > 0.5,
                             human_gt=c(aux["human_mask"])[:P].view(sh), ignore_mask_list=STREET_DEPTH["ignore_mask_list"],
                             mask_pred_thresh=0.5, mask_erode=1)
    kw = dict(fn_type="l2", gt_pre_scale=80.0, gt_pre_shift=1.0, alpha_grad_reg=1.0e-2, grad_reg_scales=4, w=1.0e-4)
    gt = c(aux["depth"])[:P].view(sh)
    r32, r64 = _ref_run(lambda d_, p: ref.ssi_depth(p, gt, remain, d_, **kw), [c(main["depth_volume"])[:P].view(sh)])
    _check("ssi depth", "street depth", [parts["loss_mono_depth.depth"], parts["loss_mono_depth.reg"]], [], (r32[0], []), (r64[0], []))
    # the normals read the JOINT rendering either way (mono.py:494-500), rotated into every ray's camera frame
    N = r["mask_volume"].shape[0]
    rm = ref.remain_mask(c(r["mask_volume"]), human_gt=c(aux["human_mask"]), ignore_mask_list=STREET_NORMALS["ignore_mask_list"],
                         mask_pred_thresh=0.95, for_normals=True)
    rot = c(tr.current_c2w())[c(aux["fidx"]), :3, :3].transpose(-1, -2)
    n32, n64 = _ref_run(lambda d_, p: ref.normal_cue(p, c(aux["normals"]), rm, d_, rot=rot, w_l1=0.01, w_cos=0.01), [c(r["normals_volume"])])
    assert rm.shape == (N,)
    _check("normal cue", "street normals", [parts["loss_mono_normal.l1"], parts["loss_mono_normal.cos"]], [], (n32[0], []), (n64[0], []))


def test_trainer_mono_block_refusals(backend):
    with pytest.raises(NotImplementedError, match="points"):
        _indoor(backend, dict(mono_normals=dict(loss_per="points")))
    with pytest.raises(TypeError, match="'w_depth'"):
        _indoor(backend, dict(mono_depth=dict(w_depth=0.1)))
    with pytest.raises(ValueError, match="mask_erode > 0 needs an image patch"):
        _indoor(backend, dict(mono_normals=dict(mask_erode=2, apply_in_pixel_train_step=True, ignore_mask_list=[])))
    with pytest.raises(ValueError, match="human_mask"):
        _indoor(backend, dict(mono_depth=dict(ignore_mask_list=["human"])))
    with pytest.raises(ValueError, match="target_masks"):
        _indoor(backend, dict(mono_normals=dict(ignore_mask_list=["not_occupied"])))
    with pytest.raises(NotImplementedError, match="mono_albedo"):
        _indoor(backend, dict(mono_albedo=dict(w=1.0)))


# ------------------------------------------------------------------------------------------------ 9. the reference's own classes
# tests/golden/make_mono_loss_fixture.py runs MonoDepthLoss and MonoNormalLoss of app/loss/mono.py (loaded unchanged; erosion and
# Pearson by the restated stand-ins) on ``fixture_inputs`` and freezes losses, remain masks and gradients.  The replay reads only
# the fixture.
FIX_HW = (17, 33)
FIX_FAR = 6.0
FIX_DEPTH = {
    "indoor_l2": dict(REPLICA_DEPTH, enable_after=0, mask_erode=2),                          # the empty list keeps every pixel
    "indoor_l2_eroded": dict(REPLICA_DEPTH, enable_after=0, mask_erode=2, ignore_mask_list=["pred_not_occupied"]),
    "l1_gt_to_pred": dict(fn_type="l1", w=0.5, w_grad_reg=0.005, scale_gt_to_pred=True, ignore_mask_list=["pred_not_occupied", "toofar"],
                          mask_pred_thresh=0.5),
    "pearson": dict(w=0.3, loss_type="pearson", loss_param=dict(alpha_grad_reg=0.01, grad_reg_scales=4),
                    ignore_mask_list=["pred_not_occupied", "mono_distant"], mask_pred_thresh=0.5),
    "street": dict(STREET_DEPTH, enable_after=0, mask_erode=1),
}
FIX_NORMALS = dict(STREET_NORMALS)


def fixture_inputs():
    g = torch.Generator().manual_seed(2024)
    H, W = FIX_HW
    maps = _mask_inputs(H, W, 2024)
    pred = torch.rand(H, W, generator=g) * 5.0 + 0.5
    gt = 0.3 * pred + 0.1 + 0.05 * torch.randn(H, W, generator=g)
    mean = float(gt.double().mean())
    gt[(gt - mean).abs() < 2e-3 * mean] += 0.01
    mask_volume = torch.rand(H, W, generator=g) * 0.6 + 0.42
    mask_volume = torch.where((mask_volume - 0.5).abs() < 1e-3, mask_volume + 0.01, mask_volume)
    mask_volume = torch.where((mask_volume - 0.95).abs() < 1e-3, mask_volume + 0.01, mask_volume)
    cr_mask = mask_volume * (0.7 + 0.3 * torch.rand(H, W, generator=g))
    cr_mask = torch.where((cr_mask - 0.5).abs() < 1e-3, cr_mask + 0.01, cr_mask)
    return dict(depth_volume=pred, depth_gt=gt, mask_volume=mask_volume, cr_depth=pred * (0.9 + 0.1 * torch.rand(H, W, generator=g)),
                cr_mask=cr_mask, occupancy=maps["occupancy_gt"], human=maps["human_gt"], dynamic=maps["dynamic_gt"],
                normals_volume=torch.randn(H, W, 3, generator=g), normals_gt=torch.randn(H, W, 3, generator=g) * 0.7,
                rot=_rotations(1, g)[0])


def _depth_block(block, inp, dev):
    """``MonoDepthLoss.forward`` on the ops, as ``RenderTrainer._mono_terms`` composes it: -> (remain, terms)"""
    c = losses.mono_depth_cfg(block)
    t = lambda k: inp[k].to(dev)          # noqa: E731
    depth0 = t("depth_volume")
    if c["distant_mode"] == "cr_only":
        mask_volume, depth = t("cr_mask"), t("cr_depth")
    else:
        mask_volume, depth = t("mask_volume"), (depth0.clamp_max(FIX_FAR) if c["distant_mode"] == "clamp_far" else depth0)
    remain = losses.mono_remain_mask(mask_volume, depth_pred0=depth0, depth_pred=depth, depth_gt=t("depth_gt"), occupancy_gt=t("occupancy"),
                                     dynamic_gt=t("dynamic"), human_gt=t("human"), far=FIX_FAR, ignore_mask_list=c["ignore_mask_list"],
                                     mask_pred_thresh=c["mask_pred_thresh"], mask_erode=c["mask_erode"])
    fn = losses.mono_depth_ssi_loss if c["loss_type"] == "monosdf" else losses.mono_depth_pearson_loss
    return remain, c, (lambda p: fn(p, t("depth_gt"), remain, w=c["w"], **c["loss_param"]))


def test_reference_classes_replayed_from_the_fixture(backend):
    fx = torch.load(FIXTURE)
    inp, out = fx["inputs"], fx["outputs"]
    mine = fixture_inputs()
    assert all(torch.equal(inp[k], mine[k]) for k in mine)            # the generator ran on these very inputs
    for name, block in FIX_DEPTH.items():
        o = out[f"depth.{name}"]
        remain, c, op = _depth_block(block, inp, backend)
        assert torch.equal(remain.cpu(), o["remain"]), name
        lp = dict(c["loss_param"])
        src = "cr_depth" if c["distant_mode"] == "cr_only" else "depth_volume"
        if c["loss_type"] == "monosdf":
            rf = lambda d_, p: ref.ssi_depth(p, inp["depth_gt"], o["remain"], d_, w=c["w"], **lp)          # noqa: E731
        else:
            rf = lambda d_, p: ref.pearson_depth(p, inp["depth_gt"], o["remain"], d_, w=c["w"], **lp)      # noqa: E731
        r32, r64 = _ref_run(rf, [inp[src]])
        vals, grads = _op_run(op, [inp[src]], backend)
        frozen = ([o["losses"][k] for k in ("loss_mono_depth.depth", "loss_mono_depth.reg") if k in o["losses"]], o["grads"])
        assert len(frozen[0]) == len(vals)
        _check("ssi depth" if c["loss_type"] == "monosdf" else "pearson depth", f"replay depth.{name}", vals, grads, r32, r64, mult=2.0,
               target=frozen, unit=0.0 if c["loss_type"] == "monosdf" else 0.3 * 0.01)
    o = out["normals"]
    n = losses.mono_normals_cfg(FIX_NORMALS)
    t = lambda k: inp[k].to(backend)          # noqa: E731
    remain = losses.mono_remain_mask(t("mask_volume"), occupancy_gt=t("occupancy"), human_gt=t("human"), dynamic_gt=t("dynamic"),
                                     ignore_mask_list=n["ignore_mask_list"], mask_pred_thresh=n["mask_pred_thresh"],
                                     mask_erode=n["mask_erode"], for_normals=True)
    assert torch.equal(remain.cpu(), o["remain"])
    rot_w2c = inp["rot"].t().contiguous()          # the stand-in rotates with inv=True: n' = R^T n
    r32, r64 = _ref_run(lambda d_, p: ref.normal_cue(p.reshape(-1, 3), inp["normals_gt"].reshape(-1, 3), o["remain"].reshape(-1), d_,
                                                     rot=rot_w2c, w_l1=n["w_l1"], w_cos=n["w_cos"]), [inp["normals_volume"]])
    vals, grads = _op_run(lambda p: losses.mono_normal_cue_loss(p, t("normals_gt"), remain.reshape(-1), rot=rot_w2c.to(backend),
                                                                w_l1=n["w_l1"], w_cos=n["w_cos"]), [inp["normals_volume"]], backend)
    frozen = ([o["losses"]["loss_mono_normal.l1"], o["losses"]["loss_mono_normal.cos"]], o["grads"])
    _check("normal cue", "replay normals", vals, grads, r32, r64, mult=2.0, target=frozen)


def test_zz_measured_departures():
    """prints the table of the docstring from what the cases of this run measured"""
    print("\n    op                 f32 torch value   f32 torch grad    kernel value   kernel grad")
    for op, w in WORST.items():
        print(f"    {op:18s} {w[0]:.1e}            {w[1]:.1e}            {w[2]:.1e}         {w[3]:.1e}")
