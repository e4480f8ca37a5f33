"""Fused evaluations of the losses the object-centric training step puts on the path's outputs
and the appearance-embedding lookup, and the pointwise part of the SDF curvature regulariser (app/loss/sdf_curvature.py:42,69,75).
The reference writes these as a few torch ops each (app/loss/eikonal.py:96-105,
app/loss/photometric.py:88-146, app/models/scene/image_embeddings.py:23-80); values and gradients are identical, the
launch count is not (one kernel per direction)."""
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
