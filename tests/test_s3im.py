"""The SSIM and S3IM training losses (app/loss/perceptual.py): the ``nsim_ssim_*`` kernels in their planar and
indexed addressing, ``neuralsim_amd.losses.{ssim, s3im_loss, s3im_index}``, the shim's ``nr3d_lib.models.loss.ssim.ssim_module``, the
reference's own ``S3IMLoss`` / ``PerceptualLoss(loss_type='ssim')`` on top of it, and the trainer's ``w_s3im`` -- against the float64
restatement tests/ssim_ref.py.

Bounds.  The same formula evaluated with f32 torch ops on a CPU departs from its f64 evaluation by at most 1.8e-7 in the value and
3.8e-6 max|grad64| in the gradient on random inputs in [0, 1]; on flat bright images (0.999 - 1e-3 rand) by up to 2.4e-5 and
8.3e-4 max|grad64|, the cancellation of E[x^2] - mu^2 against C2 = 9e-4.  The asserted bounds are 5-10 x the first pair, which
leaves room for another summation order and for the float atomics of the indexed form:

    value  |ssim - ssim64| <= 2e-6          gradient  max |g - g64| <= 2e-5 max |g64|,  no element exempt.

The kernels take every moment about the window mean and every difference between inputs (csrc/loss_ops.hip), so the flat bright and
flat dark cases meet the SAME bounds (emulator: value 1.0e-7, gradient 3.2e-7 relative) and are held to them, not to the
1e-4 / 4e-3 the textbook form would need.  A gradient compared with the frozen f32 run of tests/golden/s3im_fixture.pt gets twice the
bound: both runs lie within one bound of the float64 values."""
import math
import types
from pathlib import Path

import pytest
import torch

import ref_glue
import ssim_ref as ref
from conftest import sync
from neuralsim_amd import _lib, losses
from util import leaf

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = ROOT / "tests" / "golden" / "s3im_fixture.pt"
VAL_TOL, GRAD_TOL = 2e-6, 2e-5
needs_reference = ref_glue.needs_reference(ref_glue.readable(ref_glue.REF_ROOT / "app/loss/perceptual.py"),
                                           reason="executes the reference's own loss classes (emulator backend only); what it pins "
                                                  "is replayed from tests/golden/s3im_fixture.pt on both backends")


def _rand(shape, seed, kind="random"):
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(shape, generator=g)
    return dict(random=r, bright=0.999 - 1e-3 * r, dark=0.002 + 1e-4 * r)[kind]


def _check(tag, val, grad, val64, grad64, mult=1.0):
    ev = abs(float(val.detach()) - float(val64))
    scale = float(grad64.abs().max())
    eg = float((grad.detach().cpu().double() - grad64).abs().max())
    print(f"{tag}: value err {ev:.3e} (bound {mult * VAL_TOL:.1e}), grad err {eg / scale:.3e} max|g64| (bound {mult * GRAD_TOL:.1e})")
    assert math.isfinite(ev) and ev <= mult * VAL_TOL
    assert bool(torch.isfinite(grad).all()) and eg <= mult * GRAD_TOL * scale


# ------------------------------------------------------------------------------------------------ 1. planar
PLANAR = [((2, 3, 13, 17), 11, 1),       # heavy overlap, padding 5 on every side
          ((1, 3, 7, 27), 4, 4),         # Ho 2, Wo 7; even window, padding 1: the windows end exactly on row 6 / column 26
          ((1, 3, 8, 29), 4, 4),         # ... one row and two columns more: they belong to no window and get zero gradient
          ((1, 3, 7, 27), 3, 2),         # odd window, partial overlap
          ((1, 1, 3, 5), 11, 1)]         # image smaller than the window, C = 1


@pytest.fixture(scope="module")
def planar_refs():
    out = {}
    for i, (shape, k, s) in enumerate(PLANAR):
        x, y = _rand(shape, 10 + i), _rand(shape, 20 + i)
        v, g = ref.value_and_grad(lambda a: ref.ssim(a, y, k, s), x)
        out[(shape, k, s)] = (x, y, v, g)
    return out


@pytest.mark.parametrize("shape,k,s", PLANAR)
def test_planar_matches_float64(backend, planar_refs, shape, k, s):
    x, y, v64, g64 = planar_refs[(shape, k, s)]
    xl = leaf(x, backend)
    v = losses.ssim(xl, y.to(backend), window_size=k, stride=s)
    assert v.shape == () and v.dtype == torch.float32
    v.backward()
    sync(backend)
    assert xl.grad.shape == x.shape
    _check(f"planar {shape} k={k} s={s}", v, xl.grad, v64, g64)
    if shape == (1, 3, 8, 29):            # p = 1, Ho 2, Wo 7: the windows reach row 6 and column 26
        assert float(g64[:, :, 7, :].abs().max()) == 0.0 and float(g64[..., 27:].abs().max()) == 0.0 and float(g64[:, :, 6, 26].abs().min()) > 0
        assert torch.equal(xl.grad.cpu()[:, :, 7, :], torch.zeros(1, 3, 29)) and torch.equal(xl.grad.cpu()[..., 27:], torch.zeros(1, 3, 8, 2))
    # a non-contiguous first image takes the same path
    xt = leaf(x.transpose(2, 3).contiguous(), backend)
    v2 = losses.ssim(xt.transpose(2, 3), y.to(backend), window_size=k, stride=s)
    assert abs(float(v2.detach()) - float(v.detach())) <= VAL_TOL


# ------------------------------------------------------------------------------------------------ 2. identical / flat images
@pytest.mark.parametrize("k,s", [(4, 4), (11, 1)])
def test_identical_and_flat_images(backend, k, s):
    shape = (1, 3, 16, 16)
    for kind in ("random", "bright", "dark"):
        x = _rand(shape, 31, kind)
        xl = leaf(x, backend)
        v = losses.ssim(xl, x.clone().to(backend), window_size=k, stride=s)
        v.backward()
        sync(backend)
        assert abs(1.0 - float(v.detach())) <= 1e-6, (kind, float(v.detach()))
        assert float(xl.grad.abs().max()) <= 1e-6                     # x = y is the maximum of the map
    for kind in ("bright", "dark"):
        x, y = _rand(shape, 32, kind), _rand(shape, 33, kind)
        v64, g64 = ref.value_and_grad(lambda a: ref.ssim(a, y, k, s), x)
        xl = leaf(x, backend)
        v = losses.ssim(xl, y.to(backend), window_size=k, stride=s)
        v.backward()
        sync(backend)
        _check(f"flat {kind} k={k} s={s}", v, xl.grad, v64, g64)


# ------------------------------------------------------------------------------------------------ 3. indexed form
def _s3im_case(ph, pw, R, N, seed):
    g = torch.Generator().manual_seed(seed)
    P = ph * pw
    index = torch.cat([torch.arange(P)] + [torch.randperm(P, generator=g) for _ in range(R - 1)])
    return torch.rand([N, 3], generator=g), torch.rand([N, 3], generator=g), index


def _run_indexed(backend, pred, gt, index, hw, k, s, gout=1.0):
    pl = leaf(pred, backend)
    v = losses.s3im_loss(pl, gt.to(backend), index.to(backend), hw, kernel_size=k, stride=s)
    assert v.shape == () and v.dtype == torch.float32
    (v * gout).backward()
    sync(backend)
    return v, pl.grad


@pytest.mark.parametrize("k,s", [(4, 4), (3, 2)])
def test_indexed_matches_float64_and_planar(backend, k, s):
    ph, pw, R, N = 7, 9, 3, 80
    P = ph * pw
    pred, gt, index = _s3im_case(ph, pw, R, N, seed=41)
    index2 = index.clone()
    index2[:4] = 5                       # one row four times inside the first window (k = 4) / the first two (k = 3, s = 2)
    index2[P + 1] = 5                    # ... and once more in the row below
    for tag, idx in (("permutations", index), ("repeated row", index2)):
        v64, g64 = ref.value_and_grad(lambda a: ref.s3im(a, gt, idx, (ph, pw), k, s), pred)
        v, grad = _run_indexed(backend, pred, gt, idx, (ph, pw), k, s)
        assert grad.shape == (N, 3)
        _check(f"indexed {tag} k={k} s={s}", v, grad, v64, g64)
        assert torch.equal(grad.cpu()[P:], torch.zeros(N - P, 3))           # rows 63..79: exact zeros
        assert float(g64[P:].abs().max()) == 0.0
        # the planar kernel on the materialised virtual image
        xv = leaf(ref.virtual_image(pred, idx, (ph, pw)), backend)
        vp = 1.0 - losses.ssim(xv, ref.virtual_image(gt, idx, (ph, pw)).to(backend), window_size=k, stride=s)
        vp.backward()
        sync(backend)
        gv = ref.value_and_grad(lambda a: 1.0 - ref.ssim(a, ref.virtual_image(gt, idx, (ph, pw)), k, s), xv.detach().cpu())[1]
        _check(f"planar on the virtual image, {tag}", vp, xv.grad, v64, gv)
        assert abs(float(vp.detach()) - float(v.detach())) <= VAL_TOL
        back = torch.zeros(N, 3, dtype=torch.float64).index_add_(0, idx, xv.grad.detach().cpu().double()[0].reshape(3, -1).t())
        assert float((back - grad.cpu().double()).abs().max()) <= GRAD_TOL * float(g64.abs().max())
    if k == 4:                           # the repeated row really is accumulated: four taps of one window and one of another
        assert float(g64[5].abs().max()) > 0


def test_indexed_reference_default_size(backend):
    ph, pw, R, N = 64, 64, 10, 4096
    pred, gt, index = _s3im_case(ph, pw, R, N, seed=42)
    v64, g64 = ref.value_and_grad(lambda a: ref.s3im(a, gt, index, (ph, pw), 4, 4), pred)
    v, grad = _run_indexed(backend, pred, gt, index, (ph, pw), 4, 4)
    _check("indexed 64x64 R=10", v, grad, v64, g64)


def test_index_helper(backend):
    P, R = 63, 4
    mk = lambda: torch.Generator(device=backend).manual_seed(7)      # noqa: E731
    idx = losses.s3im_index(P, R, backend, generator=mk())
    assert idx.shape == (R * P,) and idx.dtype == torch.long and idx.device.type == backend.type
    blocks = idx.cpu().view(R, P)
    assert torch.equal(blocks[0], torch.arange(P))
    for r in range(1, R):
        assert torch.equal(blocks[r].sort().values, torch.arange(P)) and not torch.equal(blocks[r], blocks[0])
    assert not torch.equal(blocks[1], blocks[2])
    assert torch.equal(losses.s3im_index(P, R, backend, generator=mk()), idx)
    assert torch.equal(losses.s3im_index(P, 1, backend), torch.arange(P, device=backend))
    # uniform: 2400 permutations of 4 elements, chi-square over the 24 of them (23 degrees of freedom: 58 is the 99.99 % point)
    perms = losses.s3im_index(4, 2401, backend, generator=mk()).cpu().view(2401, 4)[1:]
    code = (perms * torch.tensor([64, 16, 4, 1])).sum(-1)
    counts = torch.unique(code, return_counts=True)[1].double()
    assert counts.numel() == 24
    chi2 = float(((counts - 100.0) ** 2 / 100.0).sum())
    print(f"chi-square of 2400 drawn permutations: {chi2:.1f}")
    assert chi2 < 58.0


# ------------------------------------------------------------------------------------------------ 4. upstream gradient
def test_upstream_gradient_scales_linearly(backend):
    """gout enters as one factor of the per-element scale: the two backwards differ by its rounding, the product's and -- in the
    indexed form -- the order of the R atomic adds per row: well inside 1e-6 max|grad|."""
    ph, pw, R, N = 7, 9, 3, 80
    pred, gt, index = _s3im_case(ph, pw, R, N, seed=43)
    _, g1 = _run_indexed(backend, pred, gt, index, (ph, pw), 4, 4)
    _, g2 = _run_indexed(backend, pred, gt, index, (ph, pw), 4, 4, gout=0.37)
    assert float(g1.abs().max()) > 0
    assert float((g2 - 0.37 * g1).abs().max()) <= 1e-6 * float(g1.abs().max())
    x, y = _rand((1, 3, 7, 27), 44), _rand((1, 3, 7, 27), 45)
    a, b = leaf(x, backend), leaf(x, backend)
    losses.ssim(a, y.to(backend), 3, 2).backward()
    (losses.ssim(b, y.to(backend), 3, 2) * 0.37).backward()
    sync(backend)
    assert float((b.grad - 0.37 * a.grad).abs().max()) <= 1e-6 * float(a.grad.abs().max())


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_product_refuses_host_tensors():
    from nr3d_lib.models.loss.ssim import ssim_module
    x, p = torch.rand(1, 3, 8, 8), torch.rand(16, 3)
    for f in (lambda: losses.ssim(x, x), lambda: losses.s3im_loss(p, p, torch.arange(16), (4, 4)), lambda: ssim_module()(x, x)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            f()


def test_refusals(backend):
    p, g = torch.rand(16, 3, device=backend), torch.rand(16, 3, device=backend)
    idx = torch.arange(16, device=backend)
    with pytest.raises(ValueError, match="N >= patch_h"):
        losses.s3im_loss(p[:15], g[:15], idx, (4, 4))
    with pytest.raises(NotImplementedError, match="gt.requires_grad"):
        losses.s3im_loss(p, g.clone().requires_grad_(True), idx, (4, 4))
    x = torch.rand(1, 3, 16, 16, device=backend)
    with pytest.raises(NotImplementedError, match="img2.requires_grad"):
        losses.ssim(x, x.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="window_size=13"):
        losses.ssim(x, x, window_size=13)
    with pytest.raises(NotImplementedError, match="window_size=12"):
        losses.s3im_loss(p, g, idx, (4, 4), kernel_size=12)
    with pytest.raises(ValueError):
        losses.s3im_loss(p, g, idx[:15], (4, 4))
    with pytest.raises(ValueError, match="no 4x4 window"):
        losses.ssim(x[:, :, :1], x[:, :, :1], window_size=4)           # an even window on one row: Ho = 0
    with pytest.raises(RuntimeError, match="code 55"):                   # the entry point itself
        _lib.call("nsim_ssim_fwd", _lib.ptr(x), _lib.ptr(x), None, 0, 3, 16, 16, 12, 1, _lib.ptr(x), _lib.ptr(x))


# ------------------------------------------------------------------------------------------------ 6. shim
def test_shim_module(backend):
    from nr3d_lib.models.loss.ssim import ssim_module
    loss_param = {}
    loss_param.setdefault("window_size", 11)
    loss_param.setdefault("stride", 1)
    a = ssim_module(**loss_param, device=backend)                                        # perceptual.py:61-63
    b = ssim_module(channel=3, window_size=4, stride=4, device=backend)                  # perceptual.py:142
    assert isinstance(a, torch.nn.Module) and (a.window_size, a.stride, b.window_size, b.stride) == (11, 1, 4, 4)
    assert list(a.parameters()) == [] and a.to(backend) is a
    x, y = _rand((7, 3, 24, 24), 51), _rand((7, 3, 24, 24), 52)
    for mod, k, s in ((a, 11, 1), (b, 4, 4)):
        v64, g64 = ref.value_and_grad(lambda t: ref.ssim(t, y, k, s), x)
        xl = leaf(x, backend)
        v = mod(xl, y.to(backend))
        assert v.shape == ()
        v.backward()
        sync(backend)
        _check(f"ssim_module k={k} s={s}", v, xl.grad, v64, g64)
    for kw, key in ((dict(size_average=False), "size_average"), (dict(window_size=13), "window_size"), (dict(val_range=2.0), "val_range")):
        with pytest.raises(NotImplementedError, match=key):
            ssim_module(**kw)
    with pytest.raises(ValueError):
        b(x[:, :1].to(backend), y[:, :1].to(backend))


# ------------------------------------------------------------------------------------------------ 7. the reference's classes
S3IM_CFG = dict(w=0.7, kernel_size=4, stride=4, repeat_time=3, patch_height=7, patch_width=9)
S3IM_N, REF_SEED, PERC_SHAPE, PERC_W = 80, 1234, (2, 12, 14, 3), 0.3


def reference_inputs():
    g = torch.Generator().manual_seed(61)
    return dict(pred=torch.rand([S3IM_N, 3], generator=g), gt=torch.rand([S3IM_N, 3], generator=g),
                img_pred=torch.rand(PERC_SHAPE, generator=g), img_gt=torch.rand(PERC_SHAPE, generator=g))


def reference_index():
    """the index ``S3IMLoss.forward`` draws after ``torch.manual_seed(REF_SEED)`` (perceptual.py:151-152)"""
    P = S3IM_CFG["patch_height"] * S3IM_CFG["patch_width"]
    torch.manual_seed(REF_SEED)
    return torch.cat([torch.arange(P)] + [torch.randperm(P) for _ in range(S3IM_CFG["repeat_time"] - 1)])


def perceptual_images(t):
    """(B)HWC -> BCHW as ``PerceptualLoss.loss_fn`` does it (perceptual.py:67-69)"""
    *_, H, W, C = t.shape
    return t.movedim(-3, -1).reshape(-1, C, H, W)


def run_reference_losses(dev):
    """-> dict(s3im=(loss, d rgb_volume), perceptual=(loss, d rgb_volume)) of the reference's classes, loaded unchanged"""
    inp = reference_inputs()
    scene = types.SimpleNamespace(device=dev)
    out = {}
    with ref_glue.reference_loss_module("perceptual") as mod:
        pred = leaf(inp["pred"], dev)
        s3 = mod.S3IMLoss(**S3IM_CFG, device=dev)
        torch.manual_seed(REF_SEED)
        r = s3(scene, dict(rendered=dict(rgb_volume=pred)), {}, dict(image_rgb=inp["gt"]), 0)
        assert set(r) == {"rgb_s3im"}
        r["rgb_s3im"].backward()
        out["s3im"] = (r["rgb_s3im"].detach().clone(), pred.grad.clone())
        img = leaf(inp["img_pred"], dev)
        pl = mod.PerceptualLoss(w=PERC_W, loss_type="ssim", loss_param={}, device=dev)
        r = pl(scene, dict(rendered=dict(rgb_volume=img)), {}, dict(image_rgb=inp["img_gt"]), it=0, mode="image_patch")
        assert set(r) == {"loss_ssim"}
        r["loss_ssim"].backward()
        out["perceptual"] = (r["loss_ssim"].detach().clone(), img.grad.clone())
    return out


def _float64_of_the_reference_run(inp, index):
    hw = (S3IM_CFG["patch_height"], S3IM_CFG["patch_width"])
    s3 = ref.value_and_grad(lambda a: S3IM_CFG["w"] * ref.s3im(a, inp["gt"], index, hw, S3IM_CFG["kernel_size"], S3IM_CFG["stride"]),
                            inp["pred"])
    pc = ref.value_and_grad(lambda a: PERC_W * (1.0 - ref.ssim(perceptual_images(a), perceptual_images(inp["img_gt"].double()), 11, 1)),
                            inp["img_pred"])
    return s3, pc


@needs_reference
def test_reference_loss_classes_unchanged(backend):
    """``S3IMLoss`` and ``PerceptualLoss(loss_type='ssim')`` (app/loss/perceptual.py, loaded unchanged) on the shim's ``ssim_module``:
    value and ``rgb_volume.grad`` against the float64 restatement with the same permutations (the seeded torch generator)."""
    got = run_reference_losses(backend)
    s3, pc = _float64_of_the_reference_run(reference_inputs(), reference_index())
    _check("S3IMLoss", got["s3im"][0], got["s3im"][1], *s3)
    _check("PerceptualLoss ssim", got["perceptual"][0], got["perceptual"][1], *pc)
    fx = torch.load(FIXTURE)                                         # the fixture is a frozen copy of THIS run
    assert torch.equal(fx["index"], reference_index()) and all(torch.equal(v, fx[k]) for k, v in reference_inputs().items())
    _check("S3IMLoss vs fixture", got["s3im"][0], got["s3im"][1], fx["s3im_loss"].double(), fx["s3im_grad"].double(), mult=2.0)


def test_reference_run_replayed_from_the_fixture(backend):
    """The frozen run of the test above (tests/golden/make_s3im_fixture.py: inputs, the drawn index, both losses and gradients)
    through this package's own functions: within the bound of the float64 values, within twice the bound of the frozen f32 run."""
    fx = torch.load(FIXTURE)
    inp = {k: fx[k] for k in ("pred", "gt", "img_pred", "img_gt")}
    hw = (int(fx["patch_hw"][0]), int(fx["patch_hw"][1]))
    assert hw == (S3IM_CFG["patch_height"], S3IM_CFG["patch_width"]) and fx["index"].shape[0] == S3IM_CFG["repeat_time"] * hw[0] * hw[1]
    s3, pc = _float64_of_the_reference_run(inp, fx["index"])
    pred = leaf(fx["pred"], backend)
    l = float(fx["s3im_w"]) * losses.s3im_loss(pred, fx["gt"].to(backend), fx["index"].to(backend), hw, int(fx["kernel_size"]), int(fx["stride"]))
    l.backward()
    img = leaf(fx["img_pred"], backend)
    lp = float(fx["perceptual_w"]) * (1.0 - losses.ssim(perceptual_images(img), perceptual_images(fx["img_gt"].to(backend)), 11, 1))
    lp.backward()
    sync(backend)
    _check("replay s3im vs float64", l, pred.grad, *s3)
    _check("replay perceptual vs float64", lp, img.grad, *pc)
    _check("replay s3im vs frozen run", l, pred.grad, fx["s3im_loss"].double(), fx["s3im_grad"].double(), mult=2.0)
    _check("replay perceptual vs frozen run", lp, img.grad, fx["perceptual_loss"].double(), fx["perceptual_grad"].double(), mult=2.0)


# ------------------------------------------------------------------------------------------------ 8. trainer
S3IM_TINY = dict(patch_height=4, patch_width=6, repeat_time=3, kernel_size=4, stride=2)       # 24 rays: the whole batch


def _tiny_trainer(backend, **kw):
    from test_curvature import _tiny_trainer as make
    return make(backend, **kw)


def test_trainer_s3im_term(backend):
    m, tr = _tiny_trainer(backend, w_s3im=0.5, s3im=S3IM_TINY)
    assert not tr._fused_ok()                                       # the term runs on the autograd path
    loss = tr.train_step(0)
    parts = tr.loss_parts
    assert math.isfinite(float(loss)) and "rgb_s3im" in parts and 0.0 < float(parts["rgb_s3im"]) <= 0.5 * 2.0
    want = float(parts["loss_rgb"]) + tr.w_eikonal * float(parts["loss_eikonal"]) + float(parts["rgb_s3im"])
    assert abs(float(loss) - want) <= 1e-5 * abs(want)
    g = m.encoding.flattened_params.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    m0, tr0 = _tiny_trainer(backend, fused_step=False)
    loss0 = tr0.train_step(0)
    assert "rgb_s3im" not in tr0.loss_parts and abs(float(loss0) - (want - float(parts["rgb_s3im"]))) <= 1e-4
    assert float((g - m0.encoding.flattened_params.grad).abs().max()) > 0
    from neuralsim_amd.trainer import RenderTrainer
    with pytest.raises(ValueError, match="num_rays"):
        RenderTrainer(m, tr.intr, tr.c2w, tr.WH, num_rays=24, w_s3im=0.5)               # the default 64 x 64 patch
    with pytest.raises(NotImplementedError, match="sigma"):
        RenderTrainer(m, tr.intr, tr.c2w, tr.WH, num_rays=24, w_s3im=0.5, s3im=dict(S3IM_TINY, sigma=2.0))


def test_trainer_s3im_converges_on_a_fixed_objective(backend):
    """One batch, rewound generators (util.steps_on_a_fixed_objective): the same pixels, jitter, uniform points and the same S3IM
    permutations every step, so the term is one fixed function of the parameters -- lower after 30 Adam steps than at step 0."""
    from util import steps_on_a_fixed_objective
    m, tr = _tiny_trainer(backend, w_s3im=0.5, s3im=S3IM_TINY)
    xy, fidx, gt = tr.sample_batch()
    tr.sample_batch = lambda: (xy, fidx, gt)
    term = []
    step = tr.train_step

    def recording_step(it):
        out = step(it)
        term.append(float(tr.loss_parts["rgb_s3im"]))
        return out
    tr.train_step = recording_step
    losses_ = steps_on_a_fixed_objective(tr, range(31))
    assert all(l == l for l in losses_) and len(term) == 31
    print("s3im term", ["%.5f" % c for c in term])
    assert term[-1] < term[0], term


def test_trainer_without_the_term_is_bit_identical(backend, monkeypatch):
    """``w_s3im=0`` (with or without an ``rgb_s3im`` block) is the trainer built without the arguments: the same path, the same
    C-ABI calls in the first step, nothing drawn from either generator (their states are compared bit by bit on both backends),
    the same losses and parameters after 3 steps.

    What "the same" can mean for the numbers depends on the backend.  The emulator runs its threads in a fixed order, so two runs of
    one program agree bit for bit and the two trainers are held to that.  On the device two runs of the SAME trainer do not: the
    gradient scatter and the loss reductions add floats atomically in an order that changes from run to run, and Adam normalises
    the gradients, so an entry whose gradient is rounding noise may take a different +-lr step (test_trainer.py,
    ``test_fused_step_equals_autograd_step``).  There the two trainers are held to the allowance that test gives two runs of
    identical kernels, scaled to the 3 steps taken here: losses to 1e-5 relative, all but 2e-3 of a parameter's entries within
    5e-5 + 1e-4 |p|, and no entry further apart than 2 x 3 steps x lr."""
    exact = backend.type != "cuda"
    outs = []
    for kw in (dict(), dict(w_s3im=0.0, s3im=S3IM_TINY), dict(w_s3im=0.0)):
        m, tr = _tiny_trainer(backend, **kw)
        assert tr.w_s3im == 0.0 and tr.s3im is None and tr._fused_ok() == tr.fused_step
        monkeypatch.setattr(_lib, "CALL_COUNT", 0)
        ls = [float(tr.train_step(0))]
        calls = _lib.CALL_COUNT
        monkeypatch.setattr(_lib, "CALL_COUNT", None)
        ls += [float(tr.train_step(it)) for it in (1, 2)]
        sync(backend)
        assert "rgb_s3im" not in tr.loss_parts
        outs.append((ls, [p.detach().cpu().clone() for p in tr.optim.params()], tr.gen.get_state().cpu(), tr.gen_shared.get_state().cpu(),
                     calls, sorted(tr.loss_parts)))
    a = outs[0]
    assert all(math.isfinite(l) for l in a[0]) and a[4] > 0
    for b in outs[1:]:
        assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])          # nothing was drawn
        assert a[4] == b[4] and a[5] == b[5]                                # the same launches, the same terms
        assert len(a[1]) == len(b[1]) and all(p.shape == q.shape for p, q in zip(a[1], b[1]))
        if exact:
            assert a[0] == b[0] and all(torch.equal(p, q) for p, q in zip(a[1], b[1]))
            continue
        assert all(abs(x - y) <= 1e-5 * (1 + abs(x)) for x, y in zip(a[0], b[0])), (a[0], b[0])
        for p, q in zip(a[1], b[1]):
            d = (p.float() - q.float()).abs()
            bad = d > (5e-5 + 1e-4 * p.float().abs())
            print(f"param {tuple(p.shape)}: max diff {float(d.max()):.3e}, outside the allowance {float(bad.float().mean()):.2e}")
            assert float(bad.float().mean()) < 2e-3 and float(d.max()) <= 2 * 3 * 2e-3
