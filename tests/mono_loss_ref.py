"""Torch restatement of the monocular depth / normal cue losses and of an object's share of the joint rendering, written from the
reference's app/loss/mono.py and app/renderers/single_volume_renderer.py:104-120 (and the ``share`` composition of
buffer_compose_renderer.py:266-274).  Dtype-generic: the tests run it in float64 (the reference value) and in float32 (whose
departure from float64 sets the kernels' bound).  Shares no code with neuralsim_amd/losses.py.

Unpinned readings, restated here because neither library is installed where the tests run:
  * ``kornia.morphology.erosion(x[None, None], ones([2e, 2e]))`` with its default geodesic border: ``erode`` below --
    out[y, x] = min over rows y-e .. y+e-1 and columns x-e .. x+e-1, pixels outside the image do not erode;
  * ``torchmetrics.functional.pearson_corrcoef``: ``pearson`` below, the stand-in of tests/ref_glue.py:639-641."""
import torch
import torch.nn.functional as F

IGNORE = ("toofar", "pred_not_occupied", "not_occupied", "dynamic", "human", "pred_distant", "mono_distant")
FN_TYPES = ("mse", "l2", "l1", "log_l1", "smooth_l1", "relative_l1", "mape", "smape", "relative_l2", "huber")


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ 1. remain mask
def erode(mask: torch.Tensor, e: int) -> torch.Tensor:
    """the window definition as an explicit loop: bool [H,W] -> bool [H,W]"""
    if e <= 0:
        return mask.clone()
    H, W = mask.shape
    out = torch.ones_like(mask)
    for y in range(H):
        for x in range(W):
            ok = True
            for yy in range(y - e, y + e):
                for xx in range(x - e, x + e):
                    if 0 <= yy < H and 0 <= xx < W and not bool(mask[yy, xx]):
                        ok = False
            out[y, x] = ok
    return out


def erode_fast(mask: torch.Tensor, e: int) -> torch.Tensor:
    """the same window by max-pooling the complement padded with zeros (a pixel outside the image is not ignored); checked against
    ``erode`` by the tests"""
    if e <= 0:
        return mask.clone()
    ign = (~mask).float()[None, None]
    ign = F.pad(ign, (e, e - 1, e, e - 1), value=0.0)
    return ~(F.max_pool2d(ign, kernel_size=2 * e, stride=1)[0, 0] > 0)


def remain_mask(mask_pred=None, *, depth_pred0=None, depth_pred=None, depth_gt=None, occupancy_gt=None, dynamic_gt=None, human_gt=None,
                far=None, ignore_mask_list=(), mask_pred_thresh=0.95, mask_erode=0, for_normals=False, shape=None, fast=True):
    """mono.py:358-397 (depth) / :503-528 (normals), on float32 inputs as the reference evaluates them"""
    er = erode_fast if fast else erode
    shape = shape if shape is not None else next(t.shape for t in (mask_pred, depth_pred0, depth_pred, depth_gt, occupancy_gt) if t is not None)
    mp = None if mask_pred is None else mask_pred > mask_pred_thresh
    if for_normals:
        ign = ~mp if "pred_not_occupied" in ignore_mask_list else torch.zeros(shape, dtype=torch.bool)
        if "not_occupied" in ignore_mask_list:
            ign = ign | ~occupancy_gt
        if "dynamic" in ignore_mask_list:
            ign = ign | dynamic_gt
        if "human" in ignore_mask_list:
            ign = ign | human_gt
        remain = ~ign
        return er(remain, mask_erode) if mask_erode > 0 else remain
    if len(ignore_mask_list) == 0:
        return torch.ones(shape, dtype=torch.bool)
    ign = torch.zeros(shape, dtype=torch.bool)
    if "toofar" in ignore_mask_list:
        ign |= depth_pred0 > far
    if "pred_not_occupied" in ignore_mask_list:
        ign |= ~mp
    if "not_occupied" in ignore_mask_list:
        ign |= ~occupancy_gt
    if "dynamic" in ignore_mask_list:
        ign |= dynamic_gt
    if "human" in ignore_mask_list:
        ign |= human_gt
    if "pred_distant" in ignore_mask_list:
        ign |= depth_pred > (far * 0.8)
    if "mono_distant" in ignore_mask_list:
        ign |= depth_gt > depth_gt.mean() - 1e-5
    remain = ~ign
    return er(remain, mask_erode) if mask_erode > 0 else remain


# ------------------------------------------------------------------------------------------------ 2. scale-and-shift-invariant depth
def _mean(x, mask):
    return (x * mask.to(x.dtype)).mean()          # reduce(..., 'mean'): over ALL elements


def regression(fn_type, fn_param, a, b, mask):
    p = dict(fn_param or {})
    d = a - b
    if fn_type in ("mse", "l2"):
        x = d ** 2
    elif fn_type == "l1":
        x = d.abs()
    elif fn_type == "log_l1":
        x = (torch.log((a + 1).clamp_min(1e-3)) - torch.log(b + 1)).abs()
    elif fn_type == "smooth_l1":
        x = F.smooth_l1_loss(a, b, reduction="none", beta=p.get("beta", 1.0))
    elif fn_type in ("relative_l1", "mape"):
        x = d.abs() / (b.abs() + p.get("eps", 1e-2))
    elif fn_type == "smape":
        x = d.abs() / (0.5 * (a.abs() + b.abs()) + p.get("eps", 1e-2))
    elif fn_type == "relative_l2":
        x = d ** 2 / (b ** 2 + p.get("eps", 1e-2))
    elif fn_type == "huber":
        x = F.huber_loss(a, b, reduction="none", delta=p.get("alpha", 1.0))
    else:
        raise ValueError(fn_type)
    # (a masked-out pixel's value is replaced, not multiplied: 0 x inf would be NaN -- the kernels do not evaluate it)
    return _mean(torch.where(mask, x, torch.zeros_like(x)), mask)


def scale_and_shift(pred, target, mask):
    m = mask.to(pred.dtype)
    a00, a01, a11 = (m * pred * pred).sum(), (m * pred).sum(), m.sum()
    b0, b1 = (m * pred * target).sum(), (m * target).sum()
    det = a00 * a11 - a01 * a01
    if float(det.detach()) == 0.0:
        z = torch.zeros((), dtype=pred.dtype)
        return z, z.clone(), det
    return (a11 * b0 - a01 * b1) / det, (-a01 * b0 + a00 * b1) / det, det


def image_gradient_l1(a, b, mask):
    diff = torch.where(mask, a - b, torch.zeros_like(a))
    gx = (mask[:, 1:] & mask[:, :-1]) * (diff[:, 1:] - diff[:, :-1]).abs()
    gy = (mask[1:, :] & mask[:-1, :]) * (diff[1:, :] - diff[:-1, :]).abs()
    return gx.sum() + gy.sum()


def ssi_depth(pred, gt, mask, dtype, *, fn_type="mse", fn_param=None, gt_pre_scale=1.0, gt_pre_shift=0.0, scale_gt_to_pred=False,
              detach_scale_shift=False, alpha_grad_reg=0.01, grad_reg_scales=4, w=1.0, aux=None):
    """MonoSDFDepthLoss.forward (mono.py:136-158), times w: -> (loss_depth, loss_reg | None)"""
    gt = gt.to(dtype)
    target = gt_pre_scale * gt + gt_pre_shift
    if detach_scale_shift:
        with torch.no_grad():
            scale, shift, det = scale_and_shift(pred, target, mask)
    else:
        scale, shift, det = scale_and_shift(pred, target, mask)
    if aux is not None:
        aux.update(scale=scale, shift=shift, det=det)
    if scale_gt_to_pred:
        a, b = pred, (target - shift) / scale
    else:
        a, b = scale * pred + shift, target
    loss = w * regression(fn_type, fn_param, a, b, mask)
    reg = None
    if alpha_grad_reg > 0:
        tot = torch.zeros((), dtype=dtype)
        for k in range(grad_reg_scales):
            s = 2 ** k
            tot = tot + image_gradient_l1(a[::s, ::s], b[::s, ::s], mask[::s, ::s])
        reg = w * (alpha_grad_reg * tot)
    return loss, reg


# ------------------------------------------------------------------------------------------------ 3. Pearson depth
def pearson(a, b):
    a, b = a - a.mean(), b - b.mean()
    return (a * b).sum() / (a.norm() * b.norm()).clamp_min(1e-12)


def _pearson_gradient(pred, gt, mask):
    tot = torch.zeros((), dtype=pred.dtype)
    mx = mask[:, 1:] & mask[:, :-1]
    if bool(mx.any()):
        tot = tot + (1 - pearson((pred[:, 1:] - pred[:, :-1])[mx], (gt[:, 1:] - gt[:, :-1])[mx]))
    my = mask[1:, :] & mask[:-1, :]
    if bool(my.any()):
        tot = tot + (1 - pearson((pred[1:, :] - pred[:-1, :])[my], (gt[1:, :] - gt[:-1, :])[my]))
    return tot


def pearson_depth(pred, gt, mask, dtype, alpha_grad_reg=0.01, grad_reg_scales=4, w=1.0):
    """PearsonCorrDepthLoss.forward, reverse_gt False (mono.py:222-240), times w; an empty mask: zeros (MonoDepthLoss returns no
    terms there)"""
    gt = gt.to(dtype)
    reg = None
    if alpha_grad_reg > 0:
        tot = torch.zeros((), dtype=dtype)
        for k in range(grad_reg_scales):
            s = 2 ** k
            tot = tot + _pearson_gradient(pred[::s, ::s], gt[::s, ::s], mask[::s, ::s])
        reg = w * (alpha_grad_reg * tot)
    if not bool(mask.any()):
        return pred.sum() * 0.0, (None if reg is None else pred.sum() * 0.0)
    return w * (1 - pearson(pred[mask], gt[mask])), reg


# ------------------------------------------------------------------------------------------------ 4. normal cue
def normal_cue(normals_pred, normals_gt, mask, dtype, rot=None, w_l1=1.0, w_cos=1.0):
    """MonoNormalLoss.fn behind the rotation of mono.py:507 (n' = rot n, rot constant), the means over all N of mask x"""
    gt = normals_gt.to(dtype)
    n = normals_pred
    if rot is not None:
        r = rot.to(dtype)
        n = (r * n.unsqueeze(-2)).sum(-1)           # [3,3] or [N,3,3] times [N,1,3]
    n_p, n_g = F.normalize(n, dim=-1), F.normalize(gt, dim=-1)
    l1 = (n_p - n_g).abs().sum(-1)
    cos = 1.0 - (n_p * n_g).sum(-1)
    if mask is not None:
        l1, cos = torch.where(mask, l1, torch.zeros_like(l1)), torch.where(mask, cos, torch.zeros_like(cos))
    return w_l1 * l1.mean(), w_cos * cos.mean()


# ------------------------------------------------------------------------------------------------ 5. an object's share of the joint rendering
def packed_sum(x, pack_infos):
    seg = torch.repeat_interleave(torch.arange(pack_infos.shape[0]), pack_infos[:, 1])
    idx = torch.cat([torch.arange(int(b), int(b) + int(n)) for b, n in pack_infos.tolist()] or [torch.zeros(0, dtype=torch.long)])
    out = torch.zeros([pack_infos.shape[0], *x.shape[1:]], dtype=x.dtype)
    return out.index_add(0, seg, x[idx])


def share(vw, t, rgb, nablas, pack_infos, rays_inds, N, dtype, normalized_depth=True, normalize_nablas=False):
    """the ``share`` composition (buffer_compose_renderer.py:266-274) placed at the packs' rays, the depth normalised after the
    placement (:289-291, 306-307; single_volume_renderer.py:108-112 divides the weights instead: the same number)"""
    t = t.to(dtype)
    out = {}
    m = packed_sum(vw, pack_infos)
    d = packed_sum(vw * t, pack_infos)
    out["mask_volume"] = torch.zeros([N], dtype=dtype).index_put((rays_inds,), m)
    out["depth_volume"] = torch.zeros([N], dtype=dtype).index_put((rays_inds,), d)
    if normalized_depth:
        out["depth_volume"] = out["depth_volume"] / (out["mask_volume"] + 1e-10)
    if rgb is not None:
        out["rgb_volume"] = torch.zeros([N, 3], dtype=dtype).index_put((rays_inds,), packed_sum(vw[:, None] * rgb, pack_infos))
    if nablas is not None:
        nb = F.normalize(nablas.clamp(-1, 1), dim=-1) if normalize_nablas else nablas
        out["normals_volume"] = torch.zeros([N, 3], dtype=dtype).index_put((rays_inds,), packed_sum(vw[:, None] * nb, pack_infos))
    return out
