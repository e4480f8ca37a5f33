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


# ------------------------------------------------------------------------------------------------ monocular depth / normal cues
# The full ``mono_depth`` / ``mono_normals`` blocks (app/loss/mono.py; lotd_neus.replica.230814.yaml:272-288, withmask_nolidar.240219.yaml:
# 463-483) on the kernels of csrc/loss_ops.hip: the remain mask with its erosion in one launch, the depth losses in
# at most two launches forward and one backward, the normal cue in one per direction.  ``mono_depth_loss`` / ``mono_normal_loss``
# above stay the plain-torch core they were.
MONO_IGNORE = {"toofar": 1, "pred_not_occupied": 2, "not_occupied": 4, "dynamic": 8, "human": 16, "pred_distant": 32, "mono_distant": 64}
_MONO_NORMAL_IGNORE = ("pred_not_occupied", "not_occupied", "dynamic", "human")     # the entries MonoNormalLoss.forward looks at
MONO_MAX_ERODE = 32          # MONO_MAX_ERODE of csrc/loss_ops.hip
MONO_MAX_SCALES = 8          # MONO_MAX_SCALES


def _u8(t: torch.Tensor, name: str) -> torch.Tensor:
    _lib.require_device(t, name)
    t = t.detach()
    if t.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"neuralsim_amd: {name} must be a bool or uint8 map, got {t.dtype}")
    return t.reshape(-1).contiguous().view(torch.uint8)


def mono_remain_mask(mask_pred: torch.Tensor = None, *, depth_pred0: torch.Tensor = None, depth_pred: torch.Tensor = None,
                     depth_gt: torch.Tensor = None, occupancy_gt: torch.Tensor = None, dynamic_gt: torch.Tensor = None,
                     human_gt: torch.Tensor = None, far: float = None, ignore_mask_list=(), mask_pred_thresh: float = 0.95,
                     mask_erode: int = 0, for_normals: bool = False, shape=None) -> torch.Tensor:
    """The pixels the monocular losses keep, bool [H,W] or [N] (no gradient): ``MonoDepthLoss.forward`` (app/loss/mono.py:358-397)
    or, ``for_normals=True``, ``MonoNormalLoss.forward`` (:503-528).  A pixel is ignored by any listed rule: ``toofar`` depth_pred0 >
    far | ``pred_not_occupied`` not (mask_pred > mask_pred_thresh) | ``not_occupied`` ~occupancy_gt | ``dynamic`` | ``human`` |
    ``pred_distant`` depth_pred > 0.8 far | ``mono_distant`` depth_gt > mean(depth_gt) - 1e-5 (the mean on the device, one extra
    launch).  A map a listed rule needs and that is missing is a ``ValueError``.  Two quirks of the reference are kept: the DEPTH loss
    with an empty list keeps every pixel, erosion or not (:396-397); the NORMAL loss always builds the mask, erodes it, and looks at
    four entries only (pred_not_occupied, not_occupied, dynamic, human -- another known entry is accepted and has no effect).
    ``mask_erode`` e > 0 (at most 32; needs a 2-D shape): ``kornia.morphology.erosion`` with a flat 2e x 2e kernel of ones, read as
    out[y,x] = min over rows y-e .. y+e-1 and columns x-e .. x+e-1, pixels outside the image not eroding (unpinned).
    One launch.  ``shape``: of the result when no map is handed in (empty list)."""
    names = list(ignore_mask_list)
    for n in names:
        if n not in MONO_IGNORE:
            raise ValueError(f"neuralsim_amd: unknown ignore_mask_list entry {n!r}")
    if for_normals:
        names = [n for n in names if n in _MONO_NORMAL_IGNORE]
    keep_all = (not for_normals) and len(names) == 0
    flags = 0
    for n in names:
        flags |= MONO_IGNORE[n]
    maps = dict(mask_pred=mask_pred, depth_pred0=depth_pred0, depth_pred=depth_pred, depth_gt=depth_gt, occupancy_gt=occupancy_gt,
                dynamic_gt=dynamic_gt, human_gt=human_gt)
    needs = {1: ("depth_pred0",), 2: ("mask_pred",), 4: ("occupancy_gt",), 8: ("dynamic_gt",), 16: ("human_gt",), 32: ("depth_pred",),
             64: ("depth_gt",)}
    for bit, ms in needs.items():
        for m in ms:
            if (flags & bit) and maps[m] is None:
                raise ValueError(f"neuralsim_amd: ignore_mask_list entry {[k for k, v in MONO_IGNORE.items() if v == bit][0]!r} needs {m}")
    if (flags & (1 | 32)) and far is None:
        raise ValueError("neuralsim_amd: ignore_mask_list entries 'toofar' / 'pred_distant' need far")
    given = [m for m in maps.values() if m is not None]
    if shape is None:
        if not given:
            raise ValueError("neuralsim_amd: mono_remain_mask needs a map or a shape")
        shape = tuple(given[0].shape)
    shape = tuple(int(s) for s in shape)
    n = 1
    for s_ in shape:
        n *= s_
    for k, m in maps.items():
        if m is not None and m.numel() != n:
            raise ValueError(f"neuralsim_amd: {k} {tuple(m.shape)} does not have the {n} pixels of {shape}")
    e = int(mask_erode)
    if e < 0 or e > MONO_MAX_ERODE:
        raise NotImplementedError(f"neuralsim_amd: mask_erode={mask_erode}: the erosion kernel takes 0..{MONO_MAX_ERODE}")
    if e > 0 and len(shape) != 2:
        raise ValueError(f"neuralsim_amd: mask_erode > 0 needs a 2-D [H,W] shape, got {shape}")
    H, W = (shape if len(shape) == 2 else (1, n))
    fl = {k: (None if maps[k] is None else _flat(maps[k], k)) for k in ("mask_pred", "depth_pred0", "depth_pred", "depth_gt")}
    u8 ={k: (None if maps[k] is None else _u8(maps[k], k)) for k in ("occupancy_gt", "dynamic_gt", "human_gt")}
    dev = next((t.device for t in given), None)
    if dev is None:
        raise ValueError("neuralsim_amd: mono_remain_mask without a map needs one to name the device")
    gsum = None
    if flags & 64:
        gsum = torch.zeros([1], dtype=torch.float64, device=dev)
        _lib.call("nsim_mono_sum_f64", _lib.ptr(fl["depth_gt"]), n, _lib.ptr(gsum))
    out = torch.empty([n], dtype=torch.uint8, device=dev)
    farv = 0.0 if far is None else float(far)
    _lib.call("nsim_mono_remain_mask", _lib.ptr(fl["mask_pred"]), _lib.ptr(fl["depth_pred0"]), _lib.ptr(fl["depth_pred"]),
              _lib.ptr(fl["depth_gt"]), _lib.ptr(u8["occupancy_gt"]), _lib.ptr(u8["dynamic_gt"]), _lib.ptr(u8["human_gt"]), _lib.ptr(gsum),
              H, W, _f32(mask_pred_thresh), _f32(farv), _f32(farv * 0.8), flags, int(keep_all), 0 if keep_all else e, _lib.ptr(out))
    return out.view(torch.bool).reshape(shape)


_SSI_FNS = {"mse": (0, None, 0.0), "l2": (0, None, 0.0), "l1": (1, None, 0.0), "log_l1": (2, None, 0.0), "smooth_l1": (3, "beta", 1.0),
            "relative_l1": (4, "eps", 1e-2), "mape": (4, "eps", 1e-2), "smape": (5, "eps", 1e-2), "relative_l2": (6, "eps", 1e-2),
            "huber": (7, "alpha", 1.0)}


def _depth_images(pred, gt, mask, what):
    _lib.require_device(pred, "pred")
    _lib.require_device(gt, "gt")
    if pred.dim() != 2 or gt.shape != pred.shape or mask.shape != pred.shape:
        raise ValueError(f"neuralsim_amd: {what} takes pred, gt, mask of one [H,W] shape, got {tuple(pred.shape)}, {tuple(gt.shape)}, "
                         f"{tuple(mask.shape)}")
    if pred.numel() == 0:
        raise ValueError(f"neuralsim_amd: {what} of an empty image")
    if gt.requires_grad:
        raise NotImplementedError(f"neuralsim_amd: gt.requires_grad: {what} differentiates the prediction only")
    return pred.detach().float().contiguous(), gt.detach().float().contiguous(), _u8(mask, "mask")


class _MonoSsiFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, mask, cfg):
        import ctypes
        p, g, m = _depth_images(pred, gt, mask, "mono_depth_ssi_loss")
        H, W = p.shape
        ws = torch.zeros([12], dtype=torch.float64, device=p.device)
        out = torch.empty([2], dtype=torch.float32, device=p.device)
        gd, gr = torch.empty_like(p), torch.empty_like(p)
        _lib.call("nsim_mono_ssi_moments", ctypes.byref(cfg), _lib.ptr(p), _lib.ptr(g), _lib.ptr(m), H, W, _lib.ptr(ws))
        _lib.call("nsim_mono_ssi_fwd", ctypes.byref(cfg), _lib.ptr(p), _lib.ptr(g), _lib.ptr(m), H, W, _lib.ptr(ws), _lib.ptr(out),
                  _lib.ptr(gd), _lib.ptr(gr))
        ctx.saved = (p, g, m, ws, gd, gr)
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g0, g1):
        import ctypes
        p, g, m, ws, gd, gr = ctx.saved
        go = [None if x is None else x.float().reshape(1).contiguous() for x in (g0, g1)]
        d = torch.empty_like(p)
        _lib.call("nsim_mono_ssi_bwd", ctypes.byref(ctx.cfg), _lib.ptr(p), _lib.ptr(g), _lib.ptr(m), p.shape[0], p.shape[1], _lib.ptr(ws),
                  _lib.ptr(gd), _lib.ptr(gr), _lib.ptr(go[0]), _lib.ptr(go[1]), _lib.ptr(d))
        return d, None, None, None


def mono_depth_ssi_loss(pred: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor, *, fn_type: str = "mse", fn_param: dict = None,
                        gt_pre_scale: float = 1.0, gt_pre_shift: float = 0.0, scale_gt_to_pred: bool = False,
                        detach_scale_shift: bool = False, alpha_grad_reg: float = 0.01, grad_reg_scales: int = 4, w: float = 1.0):
    """``MonoSDFDepthLoss.forward`` (app/loss/mono.py:136-158) on one patch, pred / gt [H,W], mask bool [H,W]: -> (loss_depth,
    loss_reg | None), both times ``w``.  target = gt_pre_scale gt + gt_pre_shift; (scale, shift) = the masked least-squares fit of the
    prediction to it (det == 0: both 0); loss_depth = mean over ALL H W of mask f(scale pred + shift, target) -- or f(pred, (target -
    shift) / scale) with ``scale_gt_to_pred`` --, f = mse | l2 | l1 | log_l1 | smooth_l1 (beta) | relative_l1 | mape | smape |
    relative_l2 (eps) | huber (alpha) as nr3d_lib/models/loss/recon.py; loss_reg = alpha_grad_reg x the summed L1 of the x- and y-
    differences of mask (a - b) on the ::2^k sub-images, k < grad_reg_scales, over the pairs with both mask pixels set
    (``alpha_grad_reg == 0``: None).  The gradient goes to ``pred``, THROUGH the solve unless ``detach_scale_shift`` (DESIGN.md
    sec. 7).  Masked-out pixels are not evaluated (the reference multiplies whatever they give by 0).  An empty mask gives zeros
    with zero gradients, without a read-back (the reference returns no terms after ``.any()``).  Two launches forward, one backward."""
    if fn_type not in _SSI_FNS:
        raise NotImplementedError(f"neuralsim_amd: mono depth fn_type={fn_type!r}")
    code, key, default = _SSI_FNS[fn_type]
    fp = dict(fn_param or {})
    _only_keys(fp, (key,) if key else (), f"mono_depth_ssi_loss(fn_param) of fn_type={fn_type!r}")
    if not 0 <= int(grad_reg_scales) <= MONO_MAX_SCALES:
        raise NotImplementedError(f"neuralsim_amd: grad_reg_scales={grad_reg_scales}: the kernels take 0..{MONO_MAX_SCALES}")
    cfg = _lib.MonoSsi()
    cfg.fn, cfg.fn_param = code, float(fp.get(key, default)) if key else 0.0
    cfg.scale_gt_to_pred, cfg.detach_scale_shift = int(bool(scale_gt_to_pred)), int(bool(detach_scale_shift))
    cfg.grad_reg_scales = int(grad_reg_scales)
    cfg.gt_pre_scale, cfg.gt_pre_shift, cfg.alpha_grad_reg, cfg.w = float(gt_pre_scale), float(gt_pre_shift), float(alpha_grad_reg), float(w)
    depth, reg = _MonoSsiFn.apply(pred, gt, mask, cfg)
    return depth, (reg if alpha_grad_reg > 0 else None)


class _MonoPearsonFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, mask, alpha, scales, w):
        p, g, m = _depth_images(pred, gt, mask, "mono_depth_pearson_loss")
        ws = torch.zeros([6 * (1 + 2 * MONO_MAX_SCALES) + 1], dtype=torch.float64, device=p.device)
        out = torch.empty([2], dtype=torch.float32, device=p.device)
        _lib.call("nsim_mono_pearson_fwd", _lib.ptr(p), _lib.ptr(g), _lib.ptr(m), p.shape[0], p.shape[1], alpha, scales, w, _lib.ptr(ws),
                  _lib.ptr(out))
        ctx.saved, ctx.args = (p, g, m, ws), (alpha, scales, w)
        ctx.set_materialize_grads(False)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g0, g1):
        p, g, m, ws = ctx.saved
        go = [None if x is None else x.float().reshape(1).contiguous() for x in (g0, g1)]
        d = torch.empty_like(p)
        _lib.call("nsim_mono_pearson_bwd", _lib.ptr(p), _lib.ptr(g), _lib.ptr(m), p.shape[0], p.shape[1], *ctx.args, _lib.ptr(ws),
                  _lib.ptr(go[0]), _lib.ptr(go[1]), _lib.ptr(d))
        return d, None, None, None, None, None


def mono_depth_pearson_loss(pred: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor, alpha_grad_reg: float = 0.01,
                            grad_reg_scales: int = 4, w: float = 1.0):
    """``PearsonCorrDepthLoss.forward`` with ``reverse_gt=False`` (app/loss/mono.py:222-240; the class default ``loss_type`` of
    ``MonoDepthLoss``): -> (w (1 - r), w alpha_grad_reg sum over the ::2^k sub-images of (1 - r_x) + (1 - r_y) | None).  r is the
    Pearson correlation of pred and gt over the masked pixels, r_x / r_y that of their x- / y-differences over the pairs with both
    mask pixels set; a set without a sample adds 0, decided on the device.  r = sum(xc yc) / max(|xc| |yc|, 1e-12) on the centred
    values (the form of the tests' stand-in for ``torchmetrics.functional.pearson_corrcoef``: unpinned), the
    moments centred from f64 raw sums.  Gradient to ``pred``.  One launch per direction; an empty mask gives zeros."""
    if not 0 <= int(grad_reg_scales) <= MONO_MAX_SCALES:
        raise NotImplementedError(f"neuralsim_amd: grad_reg_scales={grad_reg_scales}: the kernels take 0..{MONO_MAX_SCALES}")
    depth, reg = _MonoPearsonFn.apply(pred, gt, mask, float(alpha_grad_reg), int(grad_reg_scales), float(w))
    return depth, (reg if alpha_grad_reg > 0 else None)


class _MonoNormalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, mask, rot, rot_mode, w_l1, w_cos):
        a, b = _rows3(pred, "normals_pred"), _rows3(gt, "normals_gt")
        N = a.shape[0]
        ws = torch.zeros([3], dtype=torch.float64, device=a.device)
        out = torch.empty([2], dtype=torch.float32, device=a.device)
        g1, g2 = torch.empty_like(a), torch.empty_like(a)
        _lib.call("nsim_mono_normal_fwd", _lib.ptr(a), _lib.ptr(b), _lib.ptr(mask), _lib.ptr(rot), rot_mode, N, w_l1, w_cos, _lib.ptr(ws),
                  _lib.ptr(out), _lib.ptr(g1), _lib.ptr(g2))
        ctx.save_for_backward(g1, g2)
        ctx.shape = pred.shape
        ctx.set_materialize_grads(False)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g0, g1):
        a, b = ctx.saved_tensors
        go = [None if x is None else x.float().reshape(1).contiguous() for x in (g0, g1)]
        d = torch.empty_like(a)
        _lib.call("nsim_mono_scale2_bwd", _lib.ptr(a), _lib.ptr(b), a.numel(), _lib.ptr(go[0]), _lib.ptr(go[1]), _lib.ptr(d))
        return d.reshape(ctx.shape), None, None, None, None, None, None


def mono_normal_cue_loss(normals_pred: torch.Tensor, normals_gt: torch.Tensor, mask: torch.Tensor = None, rot: torch.Tensor = None,
                         w_l1: float = 1.0, w_cos: float = 1.0):
    """``MonoNormalLoss.fn`` behind the camera-frame rotation (app/loss/mono.py:479-484, 507): -> (w_l1 l1, w_cos cos).
    normals_pred, normals_gt [..., 3] (N rows), mask bool [N] or None; ``rot`` the world -> camera rotation, None | [3,3] | per
    row [N,3,3], applied as n' = rot n and constant (the reference detaches the camera transform).  Both sides are normalised as
    ``F.normalize`` (v / max(|v|, 1e-12)); l1 = mean over ALL N of mask sum_c |n'_c - g_c|, cos = mean of mask (1 - n' . g).  Rows the
    mask clears are not evaluated: a zero normal there gets a zero gradient.  Gradient to ``normals_pred``; one launch per direction."""
    if normals_pred.shape != normals_gt.shape or normals_pred.shape[-1] != 3 or normals_pred.numel() == 0:
        raise ValueError(f"neuralsim_amd: mono_normal_cue_loss takes two [..., 3] tensors of one shape, got {tuple(normals_pred.shape)} "
                         f"and {tuple(normals_gt.shape)}")
    if normals_gt.requires_grad:
        raise NotImplementedError("neuralsim_amd: normals_gt.requires_grad: the normal cue differentiates the prediction only")
    N = normals_pred.numel() // 3
    m = None
    if mask is not None:
        if mask.numel() != N:
            raise ValueError(f"neuralsim_amd: mask {tuple(mask.shape)} does not have the {N} rows of the normals")
        m = _u8(mask, "mask")
    r, mode = None, 0
    if rot is not None:
        _lib.require_device(rot, "rot")
        if tuple(rot.shape) == (3, 3):
            mode = 1
        elif tuple(rot.shape) == (N, 3, 3):
            mode = 2
        else:
            raise ValueError(f"neuralsim_amd: rot must be [3,3] or [{N},3,3], got {tuple(rot.shape)}")
        r = rot.detach().float().contiguous()
    return _MonoNormalFn.apply(normals_pred, normals_gt, m, r, mode, float(w_l1), float(w_cos))


# The scene-flow losses (app/loss/flow.py; the ``flow`` block of fg_emernerf/no_gtbox_with_flow.240208.yaml) on the four flow tensors
# of a with-flow EmerNeRF query (``volume_buffer`` / ``uniform_samples`` keys flow_fwd, flow_fwd_pred_bwd, flow_bwd,
# flow_bwd_pred_fwd): one launch forward and one backward for both terms.
class _FlowLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ff, fpb, fb, bpf, w_cycle, w_sparsity):
        rows = [_rows3(t, n) for t, n in zip((ff, fpb, fb, bpf), _FLOW_KEYS)]
        S = rows[0].shape[0]
        ws = torch.zeros([3], dtype=torch.float64, device=rows[0].device)
        out = torch.empty([2], dtype=torch.float32, device=rows[0].device)
        _lib.call("nsim_flow_loss_fwd", *[_lib.ptr(r) for r in rows], S, w_cycle, w_sparsity, _lib.ptr(ws), _lib.ptr(out))
        ctx.save_for_backward(*rows)
        ctx.shapes = [t.shape for t in (ff, fpb, fb, bpf)]
        ctx.w = (w_cycle, w_sparsity)
        ctx.set_materialize_grads(False)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_cycle, g_sparsity):
        rows = ctx.saved_tensors
        if g_cycle is None and g_sparsity is None:
            return (None,) * 6
        go = [None if g is None else g.float().reshape(1).contiguous() for g in (g_cycle, g_sparsity)]
        d = [torch.empty_like(r) if need else None for r, need in zip(rows, ctx.needs_input_grad[:4])]
        _lib.call("nsim_flow_loss_bwd", *[_lib.ptr(r) for r in rows], rows[0].shape[0], ctx.w[0], ctx.w[1], _lib.ptr(go[0]),
                  _lib.ptr(go[1]), *[_lib.ptr(t) for t in d])
        return tuple(None if t is None else t.reshape(sh) for t, sh in zip(d, ctx.shapes)) + (None, None)


_FLOW_KEYS = ("flow_fwd", "flow_fwd_pred_bwd", "flow_bwd", "flow_bwd_pred_fwd")


def flow_loss(flow_fwd: torch.Tensor, flow_fwd_pred_bwd: torch.Tensor, flow_bwd: torch.Tensor, flow_bwd_pred_fwd: torch.Tensor,
              w_cycle: float = 1.0, w_sparsity: float = 1.0):
    """``FlowLoss.fn_cycle`` / ``fn_sparsity`` (app/loss/flow.py:35-55) -> (w_cycle cycle, w_sparsity sparsity) on four [..., 3]
    tensors of one shape (S rows):
      cycle    = 1/2 mean over S 3 of (flow_fwd.detach() + flow_fwd_pred_bwd)^2 + (flow_bwd.detach() + flow_bwd_pred_fwd)^2
      sparsity = 1/4 mean over S of |flow_fwd| + |flow_fwd_pred_bwd| + |flow_bwd| + |flow_bwd_pred_fwd|
    Gradient to all four; ``flow_fwd`` / ``flow_bwd`` get none from the cycle term (the reference detaches them), and a row that is
    exactly zero gets a zero gradient from its norm.  f64 sums; one launch per direction.  S == 0 returns zeros without a launch."""
    ts = (flow_fwd, flow_fwd_pred_bwd, flow_bwd, flow_bwd_pred_fwd)
    if any(t.shape != flow_fwd.shape for t in ts) or flow_fwd.dim() < 1 or flow_fwd.shape[-1] != 3:
        raise ValueError("neuralsim_amd: flow_loss takes four [..., 3] tensors of one shape, got " +
                         ", ".join(str(tuple(t.shape)) for t in ts))
    if flow_fwd.numel() == 0:
        return tuple(torch.zeros([], dtype=torch.float32, device=flow_fwd.device) for _ in range(2))
    return _FlowLossFn.apply(*ts, float(w_cycle), float(w_sparsity))


def flow_block_terms(block: dict, raw_per_obj_model: dict, uniform_samples: dict, it: int) -> dict:
    """``FlowLoss.forward`` (app/loss/flow.py:57-123) on a ``flow`` block in the yaml's own form -- ``class_name_cfgs: {Dynamic:
    {cycle: {w | anneal, on_render_ratio}, sparsity: {...}, on_render_ratio}}``, ``on_uniform_samples`` (default true),
    ``on_render_ratio`` (default 1) -- -> the weighted terms ``loss_flow_cycle.{class}.uniform`` / ``.render`` and
    ``loss_flow_sparsity.{class}.uniform`` / ``.render``.  ``raw_per_obj_model``: {id: {class_name, volume_buffer}}; an ``empty``
    buffer and a class without an entry are skipped.  A term's render ratio is its own ``on_render_ratio``, else the class's, else the
    block's.  Weights and annealed values are resolved on the host and folded into the kernels' scales: one ``flow_loss`` launch per
    direction and sample set, whatever the number of terms."""
    import copy
    from nr3d_lib.models.annealers import get_anneal_val
    blk = dict(block)
    classes = blk.get("class_name_cfgs", {})
    on_uniform, ratio = bool(blk.get("on_uniform_samples", True)), blk.get("on_render_ratio", 1.0)
    out = {}

    def weight(config, term, cname):
        if term not in config:
            return 0, {}
        c = dict(config.pop(term))
        w = c.pop("w", None)
        if c.get("anneal", None) is not None:
            w = get_anneal_val(it=it, **c["anneal"])
        if w is None:
            raise ValueError(f"neuralsim_amd: loss_cfg flow.class_name_cfgs.{cname}.{term} has neither w nor anneal")
        return w, c

    def emit(inputs, cname, where, w_cycle, w_sparsity):
        cyc, spa = flow_loss(*inputs, w_cycle=w_cycle or 0.0, w_sparsity=w_sparsity or 0.0)
        if w_cycle is not None:
            out[f"loss_flow_cycle.{cname}.{where}"] = cyc
        if w_sparsity is not None:
            out[f"loss_flow_sparsity.{cname}.{where}"] = spa
    for obj in raw_per_obj_model.values():
        vb = obj["volume_buffer"]
        cname = obj["class_name"]
        if vb["type"] == "empty" or cname not in classes:
            continue
        config = copy.deepcopy(dict(classes[cname]))
        w_cycle, cfg_cycle = weight(config, "cycle", cname)
        w_sparsity, cfg_sparsity = weight(config, "sparsity", cname)
        on = lambda w, s=1.0: (w * s) if w > 0 else None         # noqa: E731  (a term of weight 0 is not emitted)
        if on_uniform:
            if cname not in uniform_samples:
                raise ValueError(f"neuralsim_amd: uniform_samples should contain {cname}")
            missing = [k for k in _FLOW_KEYS if k not in uniform_samples[cname]]
            if missing:
                raise ValueError(f"neuralsim_amd: uniform_samples[{cname}] should contain {missing[0]!r}")
            if w_cycle > 0 or w_sparsity > 0:
                emit([uniform_samples[cname][k] for k in _FLOW_KEYS], cname, "uniform", on(w_cycle), on(w_sparsity))
        alpha_render = config.pop("on_render_ratio", ratio)
        if alpha_render > 0 and (w_cycle > 0 or w_sparsity > 0):
            emit([vb[k] for k in _FLOW_KEYS], cname, "render", on(w_cycle, cfg_cycle.get("on_render_ratio", alpha_render)),
                 on(w_sparsity, cfg_sparsity.get("on_render_ratio", alpha_render)))
    return out


class _PackedShareFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vw, rgb, nablas, t, pack_infos, rays_inds, N, normalized_depth, normalize_nablas):
        w, tt = _flat(vw, "vw_in_total"), _flat(t, "t")
        c = None if rgb is None else _rows3(rgb, "rgb")
        nb = None if nablas is None else _rows3(nablas, "nablas")
        pi, ri = pack_infos.long().contiguous(), rays_inds.long().contiguous()
        dev = w.device
        sc = _lib.zeros([2, N], device=dev)
        nv = int(c is not None) + int(nb is not None)
        vec = _lib.zeros([nv, N, 3], device=dev) if nv else None
        o_rgb = vec[0] if c is not None else None
        o_nrm = vec[nv - 1] if nb is not None else None
        args = (_lib.ptr(w), _lib.ptr(tt), _lib.ptr(c), _lib.ptr(nb), _lib.ptr(pi), _lib.ptr(ri), pi.shape[0], N, int(normalized_depth),
                int(normalize_nablas))
        if w.numel():                          # (packs without a sample: the zeros stand)
            _lib.call("nsim_packed_share_fwd", *args, _lib.ptr(sc[0]), _lib.ptr(sc[1]), _lib.ptr(o_rgb), _lib.ptr(o_nrm))
        ctx.args, ctx.outs = args, (sc[0], sc[1])
        ctx.shapes = (vw.shape, None if rgb is None else rgb.shape, None if nablas is None else nablas.shape)
        ctx.set_materialize_grads(False)
        # (None outputs are not allowed between tensors: absent channels come back as empty tensors and are dropped by the caller)
        e = torch.zeros([0], device=dev)
        return sc[0], sc[1], (o_rgb if o_rgb is not None else e), (o_nrm if o_nrm is not None else e)

    @staticmethod
    def backward(ctx, g_mask, g_depth, g_rgb, g_nrm):
        w, tt, c, nb = ctx.args[:4]
        gs = [None if g is None else g.float().contiguous() for g in (g_mask, g_depth, g_rgb, g_nrm)]
        if c is None:
            gs[2] = None
        if nb is None:
            gs[3] = None
        d_vw = torch.empty_like(w) if ctx.needs_input_grad[0] else None
        d_rgb = torch.empty_like(c) if (c is not None and ctx.needs_input_grad[1]) else None
        d_nb = torch.empty_like(nb) if (nb is not None and ctx.needs_input_grad[2]) else None
        if w.numel():
            _lib.call("nsim_packed_share_bwd", *ctx.args, _lib.ptr(ctx.outs[0]), _lib.ptr(ctx.outs[1]), *[_lib.ptr(g) for g in gs],
                      _lib.ptr(d_vw), _lib.ptr(d_rgb), _lib.ptr(d_nb))
        s = ctx.shapes
        return (None if d_vw is None else d_vw.reshape(s[0]), None if d_rgb is None else d_rgb.reshape(s[1]),
                None if d_nb is None else d_nb.reshape(s[2]), None, None, None, None, None, None)


def packed_share(vw_in_total: torch.Tensor, t: torch.Tensor, rgb: torch.Tensor, nablas: torch.Tensor, pack_infos: torch.Tensor,
                 rays_inds: torch.Tensor, N: int, normalized_depth: bool = True, normalize_nablas: bool = False):
    """One object's share of the joint rendering, ``SingleVolumeRenderer._volume_integration_in_total``
    (app/renderers/single_volume_renderer.py:104-120): -> (mask [N], depth [N], rgb [N,3] | None, normals [N,3] | None).  Per pack
    (``pack_infos`` [P,2], its ray ``rays_inds`` [P], the packs must cover samples that exist): mask = sum vw_in_total, depth = sum vw t
    / (mask + 1e-10) -- or sum vw t with ``normalized_depth=False`` --, rgb / normals = sum vw x; ``normalize_nablas``: the
    integrated normal is ``normalize(clamp(nablas, -1, 1))``, as the reference integrates outside training.  Rays the object does
    not hit get zeros.  Gradients to ``vw_in_total``, ``rgb`` and ``nablas``, not to ``t``.  One launch per direction."""
    N = int(N)
    if pack_infos.dim() != 2 or pack_infos.shape[1] != 2 or rays_inds.shape[0] != pack_infos.shape[0]:
        raise ValueError(f"neuralsim_amd: packed_share takes pack_infos [P,2] and rays_inds [P], got {tuple(pack_infos.shape)} and "
                         f"{tuple(rays_inds.shape)}")
    S = vw_in_total.numel()
    if t.numel() != S or (rgb is not None and rgb.numel() != 3 * S) or (nablas is not None and nablas.numel() != 3 * S):
        raise ValueError("neuralsim_amd: packed_share: t, rgb, nablas must have the samples of vw_in_total")
    if t.requires_grad:
        raise NotImplementedError("neuralsim_amd: t.requires_grad: packed_share has no gradient to the depths")
    m, d, c, nr = _PackedShareFn.apply(vw_in_total, rgb, nablas, t, pack_infos, rays_inds, N, bool(normalized_depth),
                                       bool(normalize_nablas))
    return m, d, (c if rgb is not None else None), (nr if nablas is not None else None)


def rendered_share(volume_buffer: dict, n_rays: int, device=None, with_rgb: bool = True, with_normal: bool = False,
                   normalized_depth: bool = True, training: bool = True) -> dict:
    """``packed_share`` of an object's volume buffer as a ``rendered`` dict (mask_volume, depth_volume, rgb_volume, normals_volume);
    the empty rendered dict (zeros) for an ``empty`` buffer, which names no device (pass ``device``)."""
    from .renderers.single_volume_renderer import prepare_empty_rendered
    vb = volume_buffer
    if vb["type"] == "empty" or "vw_in_total" not in vb:
        if device is None:
            raise ValueError("neuralsim_amd: rendered_share of an empty buffer needs the device")
        return prepare_empty_rendered([int(n_rays)], torch.device(device), with_rgb=with_rgb, with_normal=with_normal)
    rgb = vb["rgb"].flatten(0, -2) if (with_rgb and "rgb" in vb) else None
    nab = vb["nablas_in_world"].flatten(0, -2) if (with_normal and "nablas_in_world" in vb) else None
    m, d, c, nr = packed_share(vb["vw_in_total"].reshape(-1), vb["t"].detach().reshape(-1), rgb, nab, vb["pack_infos_collect"],
                               vb["rays_inds_collect"], n_rays, normalized_depth, normalize_nablas=not training)
    out = dict(mask_volume=m, depth_volume=d)
    dev = m.device
    if with_rgb:
        out["rgb_volume"] = c if c is not None else torch.zeros([int(n_rays), 3], dtype=torch.float32, device=dev)
    if with_normal:
        out["normals_volume"] = nr if nr is not None else torch.zeros([int(n_rays), 3], dtype=torch.float32, device=dev)
    return out


_MONO_DEPTH_KEYS = ("w", "anneal", "loss_type", "loss_param", "far", "distant_mode", "ignore_mask_list", "mask_pred_thresh", "mask_erode",
                    "debug_val_every", "enable_after")
_MONO_DEPTH_FLAT = ("fn_type", "fn_param", "gt_pre_scale", "gt_pre_shift", "detach_scale_shift", "scale_gt_to_pred", "grad_reg_scales")
_MONO_LOSS_PARAMS = {"monosdf": _MONO_DEPTH_FLAT + ("alpha_grad_reg",), "pearson": ("alpha_grad_reg", "grad_reg_scales")}
_MONO_NORMAL_KEYS = ("w_l1", "w_cos", "loss_per", "distant_mode", "ignore_mask_list", "mask_pred_thresh", "mask_erode",
                     "apply_in_pixel_train_step", "enable_after", "debug_val_every")


def mono_depth_cfg(block: dict) -> dict:
    """A ``mono_depth`` yaml block as the constructor arguments of ``MonoDepthLoss`` (app/loss/mono.py:253-269), every key present.
    Takes those keys, and the flat spelling of the shipped yamls (lotd_neus.replica.230814.yaml:272-283,
    withmask_nolidar.240219.yaml:471-483), which predates the class: ``fn_type, fn_param, gt_pre_scale, gt_pre_shift,
    detach_scale_shift, scale_gt_to_pred, grad_reg_scales`` go into the ``loss_param`` of ``loss_type: monosdf``, and ``w_grad_reg``
    is read as the weight of the ``.reg`` term itself, alpha_grad_reg = w_grad_reg / w (unpinned).  Anything
    else is refused by name."""
    blk = dict(block)
    _only_keys(blk, _MONO_DEPTH_KEYS + _MONO_DEPTH_FLAT + ("w_grad_reg",), "loss_cfg mono_depth")
    flat = {k: blk.pop(k) for k in _MONO_DEPTH_FLAT + ("w_grad_reg",) if k in blk}
    out = dict(w=1.0, anneal=None, loss_type="monosdf" if flat else "pearson", loss_param={}, far=None, distant_mode=None,
               ignore_mask_list=[], mask_pred_thresh=0.95, mask_erode=0, enable_after=0)
    out.update({k: v for k, v in blk.items() if k != "debug_val_every"})
    if out["loss_type"] not in _MONO_LOSS_PARAMS:
        raise NotImplementedError(f"neuralsim_amd: mono_depth loss_type={out['loss_type']!r}")
    lp = dict(out["loss_param"] or {})
    if flat:
        if out["loss_type"] != "monosdf":
            raise TypeError(f"neuralsim_amd: loss_cfg mono_depth: {sorted(flat)[0]!r} belongs to loss_type 'monosdf', got {out['loss_type']!r}")
        if "w_grad_reg" in flat:
            w_reg = flat.pop("w_grad_reg")
            if "alpha_grad_reg" in lp:
                raise TypeError("neuralsim_amd: loss_cfg mono_depth got both w_grad_reg and loss_param.alpha_grad_reg")
            if not out["w"]:
                raise ValueError("neuralsim_amd: loss_cfg mono_depth: w_grad_reg is relative to a non-zero w")
            lp["alpha_grad_reg"] = float(w_reg) / float(out["w"])
        dup = sorted(set(flat) & set(lp))
        if dup:
            raise TypeError(f"neuralsim_amd: loss_cfg mono_depth got {dup[0]!r} twice")
        lp.update(flat)
    _only_keys(lp, _MONO_LOSS_PARAMS[out["loss_type"]], f"loss_cfg mono_depth.loss_param of loss_type={out['loss_type']!r}")
    out["loss_param"] = lp
    if out["distant_mode"] not in (None, "clamp_far", "cr_only"):
        raise RuntimeError(f"Invalid distant_mode={out['distant_mode']}")
    out["ignore_mask_list"] = list(out["ignore_mask_list"])
    for n in out["ignore_mask_list"]:
        if n not in MONO_IGNORE:
            raise ValueError(f"neuralsim_amd: unknown ignore_mask_list entry {n!r}")
    return out


def mono_normals_cfg(block: dict) -> dict:
    """A ``mono_normals`` yaml block as the constructor arguments of ``MonoNormalLoss`` (app/loss/mono.py:426-436), every key present;
    ``loss_per: points`` is refused as the reference raises (:538-539)."""
    blk = dict(block)
    _only_keys(blk, _MONO_NORMAL_KEYS, "loss_cfg mono_normals")
    out = dict(w_l1=1.0, w_cos=1.0, loss_per="pixels", distant_mode="crdv", ignore_mask_list=["pred_not_occupied", "not_occupied", "human"],
               mask_pred_thresh=0.5, mask_erode=0, apply_in_pixel_train_step=False, enable_after=0)
    out.update({k: v for k, v in blk.items() if k != "debug_val_every"})
    if out["loss_per"] == "points":
        raise NotImplementedError("neuralsim_amd: mono_normals loss_per='points' (the reference raises NotImplementedError, mono.py:539)")
    if out["loss_per"] != "pixels":
        raise RuntimeError(f"Invalid loss_per={out['loss_per']}")
    if out["distant_mode"] not in ("crdv", "cr_only"):
        raise RuntimeError(f"Invalid distant_mode={out['distant_mode']}")
    out["ignore_mask_list"] = list(out["ignore_mask_list"])
    for n in out["ignore_mask_list"]:
        if n not in MONO_IGNORE:
            raise ValueError(f"neuralsim_amd: unknown ignore_mask_list entry {n!r}")
    return out
