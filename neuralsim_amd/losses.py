"""Fused evaluations of the losses the object-centric training step puts on the path's outputs
and the appearance-embedding lookup, and the pointwise part of the SDF curvature regulariser (app/loss/sdf_curvature.py:42,69,75).
The reference writes these as a few torch ops each (app/loss/eikonal.py:96-105,
app/loss/photometric.py:88-146, app/models/scene/image_embeddings.py:23-80); values and gradients are identical, the
launch count is not (one kernel per direction).  Likewise the supervision blocks of the street configs: occupancy mask, mask
entropy, sparsity, clearance and the lidar loss (app/loss/{mask, mask_entropy, sparsity, clearance, lidar}.py)."""
import torch

from . import _lib


class _EikonalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, nablas):
        nab = nablas.float().reshape(-1, 3).contiguous()
        out = _lib.zeros([], device=nab.device)
        _lib.call("nsim_eikonal_loss_fwd", _lib.ptr(nab), nab.shape[0], _lib.ptr(out))
        ctx.save_for_backward(nab)
        ctx.shape = nablas.shape
        return out

    @staticmethod
    def backward(ctx, g):
        nab, = ctx.saved_tensors
        d = torch.empty_like(nab)
        _lib.call("nsim_eikonal_loss_bwd", _lib.ptr(nab), nab.shape[0], _lib.ptr(g.float().contiguous()), _lib.ptr(d))
        return d.reshape(ctx.shape)


def eikonal_loss(nablas: torch.Tensor) -> torch.Tensor:
    """mean((|nablas| - 1)^2) -- ``EikonalLoss.fn(nablas).mean()`` with the defaults (no noise, plain mse)."""
    return _EikonalFn.apply(nablas)


def _rows3(t: torch.Tensor, name: str) -> torch.Tensor:
    _lib.require_device(t, name)
    return t.detach().float().reshape(-1, 3).contiguous()


class _CurvatureFn(torch.autograd.Function):
    """Saves its INPUTS only: the backward recomputes the angle, so the returned tensor -- a fresh buffer, never a view -- may be
    modified in place (``curvature.clamp_max_(0.5)``, app/loss/sdf_curvature.py:42)."""

    @staticmethod
    def forward(ctx, n0, n1):
        a, b = _rows3(n0, "n0"), _rows3(n1, "n1")
        out = torch.empty(n0.shape[:-1], dtype=torch.float32, device=a.device)
        _lib.call("nsim_curv_angle_fwd", _lib.ptr(a), _lib.ptr(b), a.shape[0], _lib.ptr(out))
        ctx.save_for_backward(a, b)
        ctx.shapes = (n0.shape, n1.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        d0 = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        d1 = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        _lib.call("nsim_curv_angle_bwd", _lib.ptr(a), _lib.ptr(b), _lib.ptr(g.float().reshape(-1).contiguous()), a.shape[0],
                  _lib.ptr(d0), _lib.ptr(d1))
        return (d0.reshape(ctx.shapes[0]) if d0 is not None else None, d1.reshape(ctx.shapes[1]) if d1 is not None else None)


def sdf_curvature(n0: torch.Tensor, n1: torch.Tensor) -> torch.Tensor:
    """``acos(clamp(n0^ . n1^, -(1 - 1e-6), 1 - 1e-6)) / pi`` per point, n^ = n / max(|n|, 1e-12): the angle between the nablas at a
    point and at its neighbour as a fraction of pi (n0, n1 [..., 3] -> [...]; the pointwise part of
    ``model.get_sdf_curvature_1d``).  Gradients to both; exactly zero where the clamp is active and for a vector
    shorter than 1e-12 (``F.normalize`` would hand back 1e12 x there)."""
    assert n0.shape == n1.shape and n0.shape[-1] == 3
    return _CurvatureFn.apply(n0, n1)


class _CurvatureLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, n0, n1, clamp_max):
        a, b = _rows3(n0, "n0"), _rows3(n1, "n1")
        out = _lib.zeros([], device=a.device)
        _lib.call("nsim_curv_loss_fwd", _lib.ptr(a), _lib.ptr(b), a.shape[0], float(clamp_max), _lib.ptr(out))
        ctx.save_for_backward(a, b)
        ctx.shapes, ctx.clamp_max = (n0.shape, n1.shape), float(clamp_max)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        d0 = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        d1 = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        _lib.call("nsim_curv_loss_bwd", _lib.ptr(a), _lib.ptr(b), a.shape[0], ctx.clamp_max, _lib.ptr(g.float().reshape(1).contiguous()),
                  _lib.ptr(d0), _lib.ptr(d1))
        return (d0.reshape(ctx.shapes[0]) if d0 is not None else None, d1.reshape(ctx.shapes[1]) if d1 is not None else None,
                None)


def sdf_curvature_loss(n0: torch.Tensor, n1: torch.Tensor, clamp_max: float = 0.5) -> torch.Tensor:
    """``mean(min(sdf_curvature(n0, n1), clamp_max))`` -- ``SDFCurvatureRegLoss.fn`` (app/loss/sdf_curvature.py:42) on the
    curvature of ``sdf_curvature``, one launch per direction."""
    assert n0.shape == n1.shape and n0.shape[-1] == 3
    return _CurvatureLossFn.apply(n0, n1, clamp_max)


class _MseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt):
        p = pred.float().contiguous()
        g = gt.float().contiguous()
        out = _lib.zeros([], device=p.device)
        _lib.call("nsim_mse_loss_fwd", _lib.ptr(p), _lib.ptr(g), p.numel(), _lib.ptr(out))
        ctx.save_for_backward(p, g)
        return out

    @staticmethod
    def backward(ctx, gout):
        p, g = ctx.saved_tensors
        d = torch.empty_like(p)
        _lib.call("nsim_mse_loss_bwd", _lib.ptr(p), _lib.ptr(g), p.numel(), _lib.ptr(gout.float().contiguous()), _lib.ptr(d))
        return d, None


def mse_loss(pred: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """mean((pred - gt)^2), gradient to ``pred`` only (the target is data)."""
    assert pred.shape == gt.shape
    return _MseFn.apply(pred, gt.detach())


SSIM_MAX_WINDOW = 11         # SSIM_MAX_WIN of csrc/loss_ops.hip


def ssim_out_hw(H: int, W: int, window_size: int, stride: int):
    """(Ho, Wo) of the SSIM map: zero padding (k - 1) // 2 on every side, stride s."""
    p = (window_size - 1) // 2
    return (H + 2 * p - window_size) // stride + 1, (W + 2 * p - window_size) // stride + 1


def _ssim_check(k, s, H, W, second, second_name):
    if not 1 <= int(k) <= SSIM_MAX_WINDOW:
        raise NotImplementedError(f"neuralsim_amd: window_size={k}: the SSIM kernels take windows of 1..{SSIM_MAX_WINDOW}")
    if int(s) < 1:
        raise ValueError(f"neuralsim_amd: stride must be >= 1, got {s}")
    if second.requires_grad:
        raise NotImplementedError(f"neuralsim_amd: {second_name}.requires_grad: the SSIM kernels differentiate the first image only")
    Ho, Wo = ssim_out_hw(H, W, int(k), int(s))
    if H < 1 or W < 1 or Ho < 1 or Wo < 1:
        raise ValueError(f"neuralsim_amd: no {k}x{k} window fits a {H}x{W} image")
    return Ho, Wo


class _SsimFn(torch.autograd.Function):
    """index None: x, y [BC,H,W] planar; else x, y [N,3] rows, the first n_rows of them gathered through index [H*W]."""

    @staticmethod
    def forward(ctx, x, y, index, n_rows, BC, H, W, k, s):
        Ho, Wo = ssim_out_hw(H, W, k, s)
        n_win = BC * Ho * Wo * (1 if index is None else 3)
        out = _lib.zeros([], device=x.device)
        coef = torch.empty([3, n_win], dtype=torch.float32, device=x.device)
        _lib.call("nsim_ssim_fwd", _lib.ptr(x), _lib.ptr(y), _lib.ptr(index), n_rows, BC, H, W, k, s, _lib.ptr(out), _lib.ptr(coef))
        ctx.save_for_backward(x, y, index, coef)
        ctx.geom = (n_rows, BC, H, W, k, s)
        return out

    @staticmethod
    def backward(ctx, g):
        x, y, index, coef = ctx.saved_tensors
        # indexed: a row is hit once per repeat of the virtual image -- atomic adds into zeros; planar: every element is stored
        d = torch.empty_like(x) if index is None else _lib.zeros(list(x.shape), device=x.device)
        _lib.call("nsim_ssim_bwd", _lib.ptr(x), _lib.ptr(y), _lib.ptr(index), *ctx.geom, _lib.ptr(coef),
                  _lib.ptr(g.float().reshape(1).contiguous()), _lib.ptr(d))
        return d, None, None, None, None, None, None, None, None


def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, stride: int = 1) -> torch.Tensor:
    """Mean SSIM of two images [B,C,H,W] in [0,1] (``ssim_module(window_size, stride)(img1, img2)`` of nr3d_lib, the pytorch-ssim
    form; definition: DESIGN.md sec. 7): Gaussian window of sigma 1.5, zero padding (k - 1) // 2, C1 = 0.01^2, C2 = 0.03^2, mean
    over all B C Ho Wo windows.  0-dim f32; one launch per direction, gradient to ``img1`` only."""
    _lib.require_device(img1, "img1")
    _lib.require_device(img2, "img2")
    if img1.dim() != 4 or img1.shape != img2.shape:
        raise ValueError(f"neuralsim_amd: ssim takes two [B,C,H,W] images of one shape, got {tuple(img1.shape)} and {tuple(img2.shape)}")
    B, C, H, W = img1.shape
    _ssim_check(window_size, stride, H, W, img2, "img2")
    if B * C == 0:
        raise ValueError("neuralsim_amd: ssim of an empty batch")
    x = img1.float().contiguous()
    out = _SsimFn.apply(x.view(B * C, H, W), img2.detach().float().contiguous().view(B * C, H, W), None, 0, B * C, H, W,
                        int(window_size), int(stride))
    return out


def s3im_index(n_pixels: int, repeat_time: int, device, generator: torch.Generator = None) -> torch.Tensor:
    """The index of S3IM's virtual image (app/loss/perceptual.py:151-152), [repeat_time * n_pixels] int64 on ``device``:
    ``arange(n_pixels)`` followed by ``repeat_time - 1`` independent uniform permutations -- the ranks of i.i.d. float64 uniforms,
    all repeats in ONE draw and one sort (the reference calls ``randperm`` per repeat; its random stream is not reproduced)."""
    ident = torch.arange(n_pixels, device=device)
    if repeat_time <= 1:
        return ident
    u = torch.rand([repeat_time - 1, n_pixels], dtype=torch.float64, device=device, generator=generator)
    return torch.cat([ident, u.argsort(dim=1).reshape(-1)])


def s3im_loss(pred: torch.Tensor, gt: torch.Tensor, index: torch.Tensor, patch_hw, kernel_size: int = 4,
              stride: int = 4) -> torch.Tensor:
    """``1 - SSIM`` of S3IM's virtual images (``S3IMLoss.forward``, app/loss/perceptual.py:145-159, without its weight): pred, gt
    [N,3] rays, P = patch_h * patch_w <= N; index [R * P] with values in [0, P) (``s3im_index``); the virtual image [3, patch_h,
    patch_w * R] holds row ``index[i * Wv + j]`` of ``pred[:P]`` / ``gt[:P]`` at (i, j) -- the flat sequence reshaped row-major.
    The image is not materialised: the kernels gather through ``index``.  Gradient to ``pred`` only; its rows from P on get
    exact zeros."""
    _lib.require_device(pred, "pred")
    _lib.require_device(gt, "gt")
    _lib.require_device(index, "index")
    ph, pw = int(patch_hw[0]), int(patch_hw[1])
    P = ph * pw
    if pred.dim() != 2 or pred.shape[1] != 3 or gt.shape != pred.shape:
        raise ValueError(f"neuralsim_amd: s3im_loss takes pred, gt [N,3], got {tuple(pred.shape)} and {tuple(gt.shape)}")
    if pred.shape[0] < P:
        raise ValueError(f"neuralsim_amd: s3im_loss needs N >= patch_h * patch_w = {P} rays, got N = {pred.shape[0]}")
    if index.dtype != torch.long or index.dim() != 1 or P < 1 or index.shape[0] % P != 0 or index.shape[0] == 0:
        raise ValueError(f"neuralsim_amd: index must be int64 [R * {P}], got {index.dtype} {tuple(index.shape)}")
    Wv = index.shape[0] // ph
    _ssim_check(kernel_size, stride, ph, Wv, gt, "gt")
    # the kernels are told P rows (an index outside them is a zero pixel); the gradient buffer is [N,3], zero from row P on
    val = _SsimFn.apply(pred.float().contiguous(), gt.detach().float().contiguous(), index.contiguous(), P, 1, ph, Wv,
                        int(kernel_size), int(stride))
    return 1.0 - val


# ------------------------------------------------------------------------------------------------ street supervision losses
# The loss blocks of the street configs beside rgb and eikonal (withmask_withlidar_joint.240219.yaml:438-500):
# app/loss/{mask, mask_entropy, sparsity, clearance, lidar}.py as one launch per direction each (the lidar loss: three forward).
# Every weight is folded into its launch, and the forward leaves the unscaled gradient, so a backward is one scale by gout.
def _f32(v) -> float:
    """the float a python scalar becomes when torch applies it to an f32 tensor"""
    import struct
    return struct.unpack("f", struct.pack("f", float(v)))[0]


def _flat(t: torch.Tensor, name: str) -> torch.Tensor:
    _lib.require_device(t, name)
    return t.detach().float().reshape(-1).contiguous()


def _only_keys(cfg: dict, allowed, what: str):
    bad = sorted(set(cfg) - set(allowed))
    if bad:
        raise TypeError(f"neuralsim_amd: {what} got an unexpected key {bad[0]!r}")


def _scale_bwd(grad: torch.Tensor, gout: torch.Tensor, shape):
    d = torch.empty_like(grad)
    _lib.call("nsim_loss_scale_bwd", _lib.ptr(grad), grad.numel(), _lib.ptr(gout.float().reshape(1).contiguous()), _lib.ptr(d))
    return d.reshape(shape)


_MASK_MODES = {None: 0, "always_occupied": 1, "only_cull_non_occupied": 2, "only_preserve_occupied": 3}


class _MaskBceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, lo, hi, mode, w):
        p = _flat(pred, "pred")
        g = _flat(gt, "gt") if gt is not None else None
        out = _lib.zeros([], device=p.device)
        err, grad = torch.empty_like(p), torch.empty_like(p)
        _lib.call("nsim_mask_bce_fwd", _lib.ptr(p), _lib.ptr(g), p.numel(), lo, hi, mode, w, _lib.ptr(out), _lib.ptr(err), _lib.ptr(grad))
        ctx.save_for_backward(grad)
        ctx.shape = pred.shape
        err = err.reshape(pred.shape)
        ctx.mark_non_differentiable(err)
        return out, err

    @staticmethod
    def backward(ctx, g, _gerr):
        grad, = ctx.saved_tensors
        return _scale_bwd(grad, g, ctx.shape), None, None, None, None, None


def mask_occupancy_loss(pred: torch.Tensor, gt: torch.Tensor, *, pred_clip: float = 1.0e-3, safe_bce: bool = True,
                        bce_limit: float = 0.1, special_mask_mode: str = None, w: float = 1.0):
    """``MaskOccupancyLoss`` (app/loss/mask.py:19-103) on ``mask_volume``: -> (loss, err).  ``loss = w * mean BCE(clamp(pred), gt)``
    with torch's -100 floor of the logs; the clamp is [bce_limit, 1 - bce_limit] (``safe_bce``, after the clip by ``pred_clip`` when
    that is > 0) or [pred_clip, 1 - pred_clip], and passes the gradient where lo <= pred <= hi.  ``special_mask_mode``:
    ``always_occupied`` (gt = 1, ``gt`` may be None), ``only_cull_non_occupied`` (the rays with gt < 0.5, against 0),
    ``only_preserve_occupied`` (gt > 0.5, against 1) -- the last two sum over their rays and divide by ALL N.  ``err [like pred] =
    |pred - gt|`` (0 outside the selection) carries no gradient.  One launch per direction; gradient to ``pred`` only."""
    if special_mask_mode not in _MASK_MODES:
        raise NotImplementedError(f"neuralsim_amd: special_mask_mode={special_mask_mode!r}")
    mode = _MASK_MODES[special_mask_mode]
    if gt is None and mode != 1:
        raise ValueError("neuralsim_amd: mask_occupancy_loss needs gt unless special_mask_mode='always_occupied'")
    if gt is not None:
        if gt.numel() != pred.numel():
            raise ValueError(f"neuralsim_amd: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in size")
        if gt.requires_grad:
            raise NotImplementedError("neuralsim_amd: gt.requires_grad: the mask loss differentiates the prediction only")
    if safe_bce:
        lo, hi = _f32(bce_limit), _f32(1.0 - bce_limit)
        if pred_clip is not None and pred_clip > 0:
            lo, hi = max(lo, _f32(pred_clip)), min(hi, _f32(1.0 - pred_clip))
    else:
        if pred_clip is None:
            raise ValueError("neuralsim_amd: safe_bce=False needs a pred_clip")
        lo, hi = _f32(pred_clip), _f32(1.0 - pred_clip)
    return _MaskBceFn.apply(pred, gt, lo, hi, mode, float(w))


class _PlaceRowsFn(torch.autograd.Function):
    """out [n] = zeros, out[idx] = vals (idx unique): the row scatter forward, the row gather backward."""

    @staticmethod
    def forward(ctx, vals, idx, n):
        v = vals.float().reshape(-1, 1).contiguous()
        out = _lib.zeros([n], device=v.device)
        _lib.call("nsim_rows_scatter_add", _lib.ptr(v), _lib.ptr(idx), idx.shape[0], 1, n, _lib.ptr(out))
        ctx.save_for_backward(idx)
        ctx.n = n
        return out

    @staticmethod
    def backward(ctx, g):
        idx, = ctx.saved_tensors
        d = torch.empty([idx.shape[0]], dtype=torch.float32, device=g.device)
        _lib.call("nsim_rows_gather", _lib.ptr(g.float().contiguous()), _lib.ptr(idx), idx.shape[0], 1, ctx.n, 0, _lib.ptr(d))
        return d, None, None


def object_mask_in_total(volume_buffer: dict, n_rays: int, device=None) -> torch.Tensor:
    """One object's share of the TOTAL rendering's opacity, [n_rays] (``volume_render_mask``, app/loss/mask_entropy.py:61-67):
    ``packed_sum(vw_in_total, pack_infos_collect)`` placed at ``rays_inds_collect``; zeros for an ``empty`` buffer (which names no
    device: pass ``device``)."""
    if volume_buffer["type"] == "empty":
        if device is None:
            raise ValueError("neuralsim_amd: object_mask_in_total of an empty buffer needs the device")
        return _lib.zeros([int(n_rays)], device=torch.device(device))
    from .graphics import pack_ops as po
    per_pack = po.packed_sum(volume_buffer["vw_in_total"].reshape(-1), volume_buffer["pack_infos_collect"])
    return _PlaceRowsFn.apply(per_pack, volume_buffer["rays_inds_collect"].contiguous(), int(n_rays))


_P, _CR, _DV = 0, 1, 2


def _ent(src, out):        # -(m log m + (1 - m) log(1 - m))
    return [(src, 0, 0, src, 0, 0, out, -1.0), (src, 1, 0, src, 1, 0, out, -1.0)]


def _cross(a, b, out, a_detach=0):        # a log b
    return [(a, 0, a_detach, b, 0, 0, out, 1.0)]


def _cross_full(a, b, out):        # a log b.data + (1 - a) log (1 - b.data)
    return [(a, 0, 0, b, 0, 1, out, 1.0), (a, 1, 0, b, 1, 1, out, 1.0)]


# mode -> (terms (a_src, a_neg, a_detach, b_src, b_neg, b_detach, out, sign), the reference's keys, does w apply); the keys are
# the reference's own, its slips included (mask_entropy.py:103, 107); :146-154 reports its two sums unweighted
MASK_ENTROPY_MODES = {
    "nop": ([], (), True),
    "crisp": (_ent(_P, 0), ("loss_mask_entropy",), True),
    "crisp_cr": (_ent(_CR, 0), ("loss_mask_entropy.crisp_cr",), True),
    "crisp_cr_0": ([(_CR, 1, 0, _CR, 1, 0, 0, -1.0)], ("loss_mask_entropy.crisp_cr",), True),
    "crisp_cr_1": ([(_CR, 0, 0, _CR, 0, 0, 0, -1.0)], ("loss_mask_entropy.crisp_cr",), True),
    "crisp_dv": (_ent(_DV, 0), ("loss_mask_entropy.crisp_dv",), True),
    "crisp_crdv": (_ent(_CR, 0) + _ent(_DV, 1), ("loss_mask_entropy.crisp_cr", "loss_mask_entropy.crisp_dv"), True),
    "crisp_cr_1_dv_0": ([(_CR, 0, 0, _CR, 0, 0, 0, -1.0), (_DV, 1, 0, _DV, 1, 0, 1, -1.0)],
                        ("loss_mask_entropy.crisp_cr", "loss_mask_entropy.crisp_dv"), True),
    "crisp_cr_0_dv_1": ([(_CR, 1, 0, _CR, 1, 0, 0, -1.0), (_DV, 0, 0, _DV, 0, 0, 1, -1.0)],
                        ("loss_mask_entropy.crisp_cr", "loss_mask_entropy.crisp_dv"), True),
    "cross_cr_on_dv": (_cross(_CR, _DV, 0), ("loss_mask_entropy.cross_cr_on_dv",), True),
    "cross_cr_detached_on_dv": (_cross(_CR, _DV, 0, 1), ("loss_mask_entropy.cross_cr_on_dv",), True),
    "cross_dv_on_cr": (_cross(_DV, _CR, 0), ("loss_mask_entropy.cross_dv_on_cr",), True),
    "cross_dv_detached_on_cr": (_cross(_DV, _CR, 0, 1), ("loss_mask_entropy.cross_dv_on_cr",), True),
    "cross_crdv": (_cross(_CR, _DV, 0) + _cross(_DV, _CR, 1),
                   ("loss_mask_entropy.cross_cr_on_dv", "loss_mask_entropy.cross_dv_on_cr"), True),
    "cross_crdv_detached": (_cross(_CR, _DV, 0, 1) + _cross(_DV, _CR, 1, 1),
                            ("loss_mask_entropy.cross_cr_on_dv", "loss_mask_entropy.cross_dv_on_cr"), True),
    "cross_cr_on_dv_detached_full": (_cross_full(_CR, _DV, 0), ("loss_mask_entropy.cross_cr_on_cr",), True),
    "cross_dv_on_cr_detached_full": (_cross_full(_DV, _CR, 0), ("loss_mask_entropy.cross_cr_on_dv",), True),
    "cross_crdv_detached_full": (_cross_full(_CR, _DV, 0) + _cross_full(_DV, _CR, 1),
                                 ("loss_mask_entropy.cross_crdv.1", "loss_mask_entropy.cross_crdv.2"), True),
    "crisp_cr_and_cross_cr_detached_on_dv": (_ent(_CR, 0) + _cross(_CR, _DV, 1, 1),
                                             ("loss_mask_entropy.crisp_cr", "loss_mask_entropy.cross_cr_on_dv"), False),
}


def _entropy_table(terms, w: float):
    tab = _lib.EntropyTable()
    tab.n_terms = len(terms)
    for k, (a, an, ad, b, bn, bd, out, sign) in enumerate(terms):
        t = tab.t[k]
        t.a_src, t.a_neg, t.a_detach, t.b_src, t.b_neg, t.b_detach, t.out, t.coef = a, an, ad, b, bn, bd, out, sign * w
    return tab


class _MaskEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tab, n_out, eps, m_pred, m_cr, m_dv):
        import ctypes
        ms = [None if m is None else _flat(m, "mask") for m in (m_pred, m_cr, m_dv)]
        first = next(m for m in ms if m is not None)
        out = _lib.zeros([2], device=first.device)
        _lib.call("nsim_mask_entropy_fwd", ctypes.byref(tab), *[_lib.ptr(m) for m in ms], first.numel(), eps, _lib.ptr(out))
        ctx.tab, ctx.eps, ctx.ms = tab, eps, ms
        ctx.shapes = [None if m is None else m.shape for m in (m_pred, m_cr, m_dv)]
        ctx.set_materialize_grads(False)
        return tuple(out[k] for k in range(n_out))

    @staticmethod
    def backward(ctx, *gouts):
        import ctypes
        ms = ctx.ms
        first = next(m for m in ms if m is not None)
        go = [None if g is None else g.float().reshape(1).contiguous() for g in gouts] + [None]
        ds = [torch.empty_like(m) if (m is not None and ctx.needs_input_grad[3 + k]) else None for k, m in enumerate(ms)]
        _lib.call("nsim_mask_entropy_bwd", ctypes.byref(ctx.tab), *[_lib.ptr(m) for m in ms], first.numel(), ctx.eps, _lib.ptr(go[0]),
                  _lib.ptr(go[1]), *[_lib.ptr(d) for d in ds])
        return (None, None, None, *[None if d is None else d.reshape(s) for d, s in zip(ds, ctx.shapes)])


def mask_entropy_loss(mode: str, *, mask_pred: torch.Tensor = None, mask_cr: torch.Tensor = None, mask_dv: torch.Tensor = None,
                      eps: float = 1.0e-5, w: float = 1.0) -> dict:
    """``MaskEntropyRegLoss.forward_code_single`` (app/loss/mask_entropy.py:45-162) for every one of its modes
    (``MASK_ENTROPY_MODES``): a dict of up to two weighted means over the rays under the reference's keys.  ``mask_pred`` is the
    total ``mask_volume``; ``mask_cr`` / ``mask_dv`` the close-range / distant object's share of the total rendering
    (``object_mask_in_total``).  Every log is of ``max(x, eps)``, which passes the gradient where x >= eps; the masks a mode detaches
    get none.  One launch per direction."""
    if mode not in MASK_ENTROPY_MODES:
        raise NotImplementedError(f"neuralsim_amd: mask_entropy mode={mode!r}")
    terms, keys, weighted = MASK_ENTROPY_MODES[mode]
    if not terms:
        return {}
    masks = (mask_pred, mask_cr, mask_dv)
    for src in sorted({t[0] for t in terms} | {t[3] for t in terms}):
        if masks[src] is None:
            raise ValueError(f"neuralsim_amd: mask_entropy mode {mode!r} needs {('mask_pred', 'mask_cr', 'mask_dv')[src]}")
    used = [m for m in masks if m is not None]
    if any(m.numel() != used[0].numel() for m in used):
        raise ValueError("neuralsim_amd: the masks of mask_entropy_loss differ in size")
    tab = _entropy_table(terms, float(w) if weighted else 1.0)
    outs = _MaskEntropyFn.apply(tab, len(keys), float(eps), mask_pred, mask_cr, mask_dv)
    return dict(zip(keys, outs))


class _PointLossFn(torch.autograd.Function):
    """sparsity / clearance: ``call`` is (entry point, its scalar arguments between M and out)"""

    @staticmethod
    def forward(ctx, x, name, args):
        v = _flat(x, "x")
        out = _lib.zeros([], device=v.device)
        grad = torch.empty_like(v)
        _lib.call(name, _lib.ptr(v), v.numel(), *args, _lib.ptr(out), _lib.ptr(grad))
        ctx.save_for_backward(grad)
        ctx.shape = x.shape
        return out

    @staticmethod
    def backward(ctx, g):
        grad, = ctx.saved_tensors
        return _scale_bwd(grad, g, ctx.shape), None, None


_SPARSITY_TYPES = {"normalized_logistic_density": (0, "inv_scale", 16.0), "normal": (1, "std", 1.0), "density_reg": (2, "lamb", 0.05)}


def sparsity_loss(x: torch.Tensor, type: str = "normalized_logistic_density", **param) -> torch.Tensor:
    """``SparsityLoss`` (app/loss/sparsity.py:47-54) on the geometry values of uniformly sampled points: ``w * mean(f(x))`` with f =
    ``normalized_logistic_density`` 4 s (1 - s), s = sigmoid(inv_scale x) (inv_scale 16) | ``normal`` exp(-x ** std) (std 1) |
    ``density_reg`` |1 - exp(-lamb x)| (lamb 0.05, sub-gradient 0 at 0).  ``param``: the function's parameter and ``w`` (1)."""
    if type not in _SPARSITY_TYPES:
        raise NotImplementedError(f"neuralsim_amd: sparsity type={type!r}")
    code, key, default = _SPARSITY_TYPES[type]
    _only_keys(param, (key, "w"), f"sparsity_loss(type={type!r})")
    if x.numel() == 0:
        raise ValueError("neuralsim_amd: sparsity_loss of no points")
    return _PointLossFn.apply(x, "nsim_sparsity_fwd", (code, float(param.get(key, default)), float(param.get("w", 1.0))))


def clearance_loss(near_sdf: torch.Tensor, beta: float = 1.0, thresh: float = 0.01, w: float = 1.0) -> torch.Tensor:
    """``ClearanceLoss.fn_penalty_sdf`` (app/loss/clearance.py:51-56): ``w * sum over near_sdf < thresh of exp(-beta (near_sdf -
    thresh)) / numel`` -- exactly zero, with a zero gradient, when no point lies below the threshold; the count of such points is
    never read back (the reference's ``.item()``)."""
    if near_sdf.numel() == 0:
        raise ValueError("neuralsim_amd: clearance_loss of no points")
    return _PointLossFn.apply(near_sdf, "nsim_clearance_fwd", (float(beta), float(thresh), float(w)))


def kth_value(x: torch.Tensor, k: int) -> torch.Tensor:
    """``torch.sort(x.flatten()).values[k]`` bit for bit, for finite non-negative f32 ``x``: one single-workgroup radix select
    (``nsim_kth_value_f32``) instead of the sort; 0-dim, stays on the device, no gradient."""
    v = _flat(x, "x")
    if not 0 <= int(k) < v.numel():
        raise ValueError(f"neuralsim_amd: kth_value needs 0 <= k < numel, got k = {k}, numel = {v.numel()}")
    out = torch.empty([], dtype=torch.float32, device=v.device)
    _lib.call("nsim_kth_value_f32", _lib.ptr(v), v.numel(), int(k), _lib.ptr(out))
    return out


_DEPTH_FNS = {"l1": 0, "l1_log": 1, "l2": 2, "l2_relative": 3, "l2_normalized": 4, "huber": 5}
_LOS_FNS = {"nerf": 1, "neus_urban": 1, "neus_unisim": 2}


def _anneal_w(cfg: dict, it: int) -> float:
    from nr3d_lib.models.annealers import get_anneal_val
    return float(cfg.get("w", 1.0)) if cfg.get("anneal") is None else float(get_anneal_val(**cfg["anneal"], it=it))


class _LidarFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, vw, cfg, mask_pred, ranges, gate, buf, aux):
        import ctypes
        d, m, r = _flat(depth, "depth_volume"), _flat(mask_pred, "mask_volume"), _flat(ranges, "ranges")
        N, dev = d.numel(), d.device
        valid = torch.empty([N], dtype=torch.uint8, device=dev)
        err = torch.empty([N], dtype=torch.float32, device=dev)
        _lib.call("nsim_lidar_valid", _lib.ptr(d), _lib.ptr(m), _lib.ptr(r), N, *gate, _lib.ptr(valid), _lib.ptr(err))
        median = None
        if cfg.factor > 0:
            median = torch.empty([], dtype=torch.float32, device=dev)
            _lib.call("nsim_kth_value_f32", _lib.ptr(err), N, N // 2, _lib.ptr(median))
        acc = _lib.zeros([3], device=dev)
        keep = torch.empty([N], dtype=torch.uint8, device=dev)
        g_depth = torch.empty([N], dtype=torch.float32, device=dev) if cfg.depth_fn >= 0 else None
        t = w_ = rih = pih = g_vw = member = None
        R = S = 0
        if buf is not None:
            t, w_ = _flat(buf["t"], "t"), _flat(vw, "vw")
            rih, pih = buf["rays_inds_hit"].long().contiguous(), buf["pack_infos_hit"].long().contiguous()
            R, S = rih.shape[0], t.numel()
            g_vw = torch.empty([S], dtype=torch.float32, device=dev)
            member = torch.empty([S], dtype=torch.uint8, device=dev)
        _lib.call("nsim_lidar_loss_fwd", ctypes.byref(cfg), _lib.ptr(d), _lib.ptr(r), _lib.ptr(valid), _lib.ptr(err), _lib.ptr(median), N,
                  _lib.ptr(t), _lib.ptr(w_), _lib.ptr(rih), _lib.ptr(pih), R, S, _lib.ptr(acc), _lib.ptr(keep), _lib.ptr(g_depth),
                  _lib.ptr(g_vw), _lib.ptr(member))
        ctx.saved = (g_depth, g_vw, member)
        ctx.shapes = (depth.shape, None if vw is None else vw.shape)
        ctx.set_materialize_grads(False)
        if aux is not None:
            aux.update(valid=valid.bool().reshape(depth.shape), err=err.reshape(depth.shape), median=median,
                       keep=keep.bool().reshape(depth.shape), member=member)
        return acc[0], acc[1], acc[2]

    @staticmethod
    def backward(ctx, g0, g1, g2):
        g_depth, g_vw, member = ctx.saved
        go = [None if g is None else g.float().reshape(1).contiguous() for g in (g0, g1, g2)]
        dd = torch.empty_like(g_depth) if (g_depth is not None and ctx.needs_input_grad[0]) else None
        dv = torch.empty_like(g_vw) if (g_vw is not None and ctx.needs_input_grad[1]) else None
        if dd is not None or dv is not None:
            _lib.call("nsim_lidar_loss_bwd", _lib.ptr(g_depth), 0 if g_depth is None else g_depth.numel(), _lib.ptr(g_vw), _lib.ptr(member),
                      0 if g_vw is None else g_vw.numel(), _lib.ptr(go[0]), _lib.ptr(go[1]), _lib.ptr(go[2]), _lib.ptr(dd), _lib.ptr(dv))
        return (None if dd is None else dd.reshape(ctx.shapes[0]), None if dv is None else dv.reshape(ctx.shapes[1]),
                None, None, None, None, None, None)


def lidar_loss(rendered: dict, volume_buffer: dict, ranges: torch.Tensor, *, depth: dict = None, line_of_sight: dict = None,
               discard_toofar: float = None, discard_outliers: float = 0, discard_outliers_median: float = 100.0,
               mask_pred_thresh: float = 1.0e-7, far: float = None, it: int = 0, toofar_replaces_mask: bool = False,
               aux: dict = None) -> dict:
    """``LidarLoss`` (app/loss/lidar.py:22-294) on a lidar render: a dict with the reference's keys ``lidar_loss.depth``,
    ``lidar_loss.los.neighbor``, ``lidar_loss.los.empty``, weights applied.  ``rendered``: ``depth_volume``, ``mask_volume`` [N];
    ``volume_buffer``: the total buffer (``packed``: t, vw, rays_inds_hit, pack_infos_hit; ``empty``: the depth term only);
    ``ranges`` [N], 0 = no return.  ``depth`` / ``line_of_sight`` are the yaml's sub-blocks (``w``, ``anneal``, ``fn_type``,
    ``fn_param``; ``epsilon_anneal`` and ``anneal`` are resolved on the host for ``it``).

    valid = (mask_volume > mask_pred_thresh) & (ranges > 0) [& (ranges <= discard_toofar)]; the final mask drops the beams whose
    |depth - ranges| valid exceeds ``discard_outliers_median`` times the median of that error over ALL N beams (``kth_value`` at
    N // 2: with more than half of the beams invalid the median is 0 and every beam with an error goes, as in the reference).  The
    reference's line :266 REPLACES the mask by the range gate; ``toofar_replaces_mask=True`` reproduces that.
    Every mean is over all N beams / all R' packs (the shim's ``reduce(.., 'mean')``).  Three launches forward, one backward;
    gradients to ``depth_volume`` and ``vw``.  ``aux``: a dict that receives ``valid``, ``err``, ``median``, ``keep``, ``member``."""
    if discard_outliers and discard_outliers > 0:
        raise NotImplementedError("neuralsim_amd: discard_outliers > 0 (a ratio of the beams: ties of an unstable sort) is not covered; "
                                  "use discard_outliers_median")
    cfg = _lib.LidarLoss()
    cfg.factor = float(discard_outliers_median or 0.0)
    cfg.depth_fn, cfg.los_fn = -1, 0
    if depth is not None:
        _only_keys(depth, ("w", "anneal", "fn_type", "fn_param"), "lidar_loss(depth=)")
        fn = depth.get("fn_type", "l1_log")
        if fn not in _DEPTH_FNS:
            raise NotImplementedError(f"neuralsim_amd: lidar depth fn_type={fn!r}")
        fp = dict(depth.get("fn_param") or {})
        _only_keys(fp, ("alpha",) if fn == "huber" else (), f"lidar_loss(depth.fn_param) of fn_type={fn!r}")
        cfg.depth_fn, cfg.w_depth = _DEPTH_FNS[fn], _anneal_w(depth, it)
        if fn == "l2_normalized":
            if far is None:
                raise ValueError("neuralsim_amd: lidar depth fn_type='l2_normalized' needs far")
            cfg.depth_param = float(far)
        elif fn == "huber":
            cfg.depth_param = float(fp.get("alpha", 1.0))
    vb_type = volume_buffer["type"]
    if vb_type not in ("packed", "empty"):
        raise NotImplementedError(f"neuralsim_amd: lidar line of sight on a volume_buffer type={vb_type!r}")
    buf, keys = None, []
    if line_of_sight is not None:
        _only_keys(line_of_sight, ("w", "anneal", "fn_type", "fn_param"), "lidar_loss(line_of_sight=)")
        fn = line_of_sight.get("fn_type", "nerf")
        if fn not in _LOS_FNS:
            raise NotImplementedError(f"neuralsim_amd: lidar line_of_sight fn_type={fn!r}")
        fp = dict(line_of_sight.get("fn_param") or {})
        if _LOS_FNS[fn] == 1:
            _only_keys(fp, ("sigma", "sigma_scale_factor"), f"lidar_loss(line_of_sight.fn_param) of fn_type={fn!r}")
            cfg.bound = float(fp.get("sigma", 1.0))
            cfg.std = cfg.bound / float(fp.get("sigma_scale_factor", 3.0))
            keys = ["lidar_loss.los.neighbor", "lidar_loss.los.empty"]
        else:
            _only_keys(fp, ("epsilon", "epsilon_anneal"), f"lidar_loss(line_of_sight.fn_param) of fn_type={fn!r}")
            eps_los = fp.get("epsilon", 1.0)
            if fp.get("epsilon_anneal") is not None:
                from nr3d_lib.models.annealers import get_anneal_val
                eps_los = get_anneal_val(**fp["epsilon_anneal"], it=it)
            cfg.bound = float(eps_los)
            keys = ["lidar_loss.los.empty"]
        if vb_type == "packed":
            cfg.los_fn, cfg.w_los, buf = _LOS_FNS[fn], _anneal_w(line_of_sight, it), volume_buffer
    toofar = float(discard_toofar) if (discard_toofar is not None and discard_toofar > 0) else 0.0
    if ranges.numel() != rendered["depth_volume"].numel():
        raise ValueError("neuralsim_amd: ranges and depth_volume differ in size")
    if ranges.requires_grad:
        raise NotImplementedError("neuralsim_amd: ranges.requires_grad: the lidar loss differentiates the rendering only")
    gate = (float(mask_pred_thresh), toofar, int(bool(toofar_replaces_mask)))
    if aux is not None:
        aux["epsilon"] = cfg.bound
    o_depth, o_nb, o_em = _LidarFn.apply(rendered["depth_volume"], None if buf is None else buf["vw"], cfg, rendered["mask_volume"],
                                         ranges, gate, buf, aux)
    out = {}
    if depth is not None:
        out["lidar_loss.depth"] = o_depth
    if buf is not None:
        for k in keys:
            out[k] = o_nb if k.endswith("neighbor") else o_em
    return out


class _EmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, idx):
        ctx.save_for_backward(idx)
        ctx.rows = table.shape[0]
        return table.detach()[idx]

    @staticmethod
    def backward(ctx, g):
        idx, = ctx.saved_tensors
        g = g.float().contiguous()
        C = g.shape[-1]
        out = _lib.zeros([ctx.rows, C], device=g.device)
        _lib.call("nsim_rows_scatter_add", _lib.ptr(g), _lib.ptr(idx), idx.shape[0], C, ctx.rows, _lib.ptr(out))
        return out, None


def embedding_lookup(table: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """``table[idx]`` (table [rows, C] f32, idx [n] int64) whose backward is one scatter-add launch instead of the
    sort-based ``index_put_(accumulate=True)`` torch falls back to."""
    assert table.dim() == 2 and idx.dim() == 1 and idx.dtype == torch.long
    return _EmbedFn.apply(table, idx.contiguous())


def mono_depth_loss(depth_pred: torch.Tensor, depth_gt: torch.Tensor, mask: torch.Tensor = None) -> torch.Tensor:
    """Scale-and-shift-invariant depth loss on one image patch (``MonoSDFDepthLoss``, app/loss/mono.py:86-157 with its
    defaults ``scale_gt_to_pred=False, detach_scale_shift=False``): the closed-form least-squares (scale, shift) that
    takes the prediction to the target -- gradients flow through the solve, as in the reference -- then the masked mse.
    Plain torch on a renderer output, as the reference does it (row a18)."""
    p, t = depth_pred.reshape(-1).float(), depth_gt.reshape(-1).float()
    m = torch.ones_like(p) if mask is None else mask.reshape(-1).to(p.dtype)
    a00, a01, a11 = (m * p * p).sum(), (m * p).sum(), m.sum()
    b0, b1 = (m * p * t).sum(), (m * t).sum()
    det = a00 * a11 - a01 * a01
    ok = det != 0
    safe = torch.where(ok, det, torch.ones_like(det))
    scale = torch.where(ok, (a11 * b0 - a01 * b1) / safe, torch.zeros_like(det))
    shift = torch.where(ok, (-a01 * b0 + a00 * b1) / safe, torch.zeros_like(det))
    return (m * (scale * p + shift - t) ** 2).sum() / m.sum().clamp_min(1.0)


def mono_normal_loss(normals_pred: torch.Tensor, normals_gt: torch.Tensor, mask: torch.Tensor = None,
                     w_l1: float = 1.0, w_cos: float = 1.0) -> torch.Tensor:
    """``MonoNormalLoss.fn`` (app/loss/mono.py:479-484): L1 + (1 - cos) between the NORMALISED rendered normals and the
    normalised prior, averaged over all pixels with the mask as weight (``reduce(..., reduction='mean')``)."""
    import torch.nn.functional as F
    n_p, n_g = F.normalize(normals_pred.reshape(-1, 3), dim=-1), F.normalize(normals_gt.reshape(-1, 3), dim=-1)
    l1 = (n_p - n_g).abs().sum(-1)
    cos = 1.0 - (n_p * n_g).sum(-1)
    if mask is not None:
        m = mask.reshape(-1).to(l1.dtype)
        l1, cos = l1 * m, cos * m
    return w_l1 * l1.mean() + w_cos * cos.mean()
