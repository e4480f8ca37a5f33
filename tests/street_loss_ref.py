"""Restatement of the street configs' supervision losses in plain torch ops (app/loss/{mask, mask_entropy,
sparsity, clearance, lidar}.py), dtype-generic: the tests evaluate it once in float64 -- the reference value -- and once in float32
on the CPU, whose departure from float64 sets the tolerance.  Gradients come from autograd.  Discrete decisions (the clamp ranges,
the validity and outlier masks, the line-of-sight membership) are taken on the float32 inputs AS float32, whatever dtype the
arithmetic then runs in: they are compared exactly, never toleranced."""
import math

import torch
import torch.nn.functional as F

from nr3d_lib.models.annealers import get_anneal_val


def f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ mask
def mask_clamp(pred_clip=1.0e-3, safe_bce=True, bce_limit=0.1):
    """(lo, hi) as float32 values: the shim's safe_binary_cross_entropy after the optional clip, or the clip alone"""
    if safe_bce:
        lo, hi = f32(bce_limit), f32(1.0 - bce_limit)
        if pred_clip is not None and pred_clip > 0:
            lo, hi = max(lo, f32(pred_clip)), min(hi, f32(1.0 - pred_clip))
        return lo, hi
    return f32(pred_clip), f32(1.0 - pred_clip)


def mask_occupancy(pred, gt, dtype, *, pred_clip=1.0e-3, safe_bce=True, bce_limit=0.1, special_mask_mode=None, w=1.0):
    """-> (loss, err); pred a leaf of ``dtype``"""
    lo, hi = mask_clamp(pred_clip, safe_bce, bce_limit)
    gt = None if gt is None else gt.to(dtype)
    n = pred.numel()
    if special_mask_mode is None or special_mask_mode == "always_occupied":
        y = torch.ones_like(pred) if special_mask_mode == "always_occupied" else gt
        loss = F.binary_cross_entropy(pred.clamp(lo, hi), y, reduction="mean")
        return w * loss, (pred.detach() - y).abs()
    sel = (gt < 0.5) if special_mask_mode == "only_cull_non_occupied" else (gt > 0.5)
    y = torch.zeros_like(pred) if special_mask_mode == "only_cull_non_occupied" else torch.ones_like(pred)
    loss = (F.binary_cross_entropy(pred.clamp(lo, hi), y, reduction="none") * sel.to(dtype)).sum() / n
    return w * loss, (pred.detach() - y).abs() * sel.to(dtype)


# ------------------------------------------------------------------------------------------------ mask entropy
def object_mask_in_total(vb, n_rays, dtype):
    mask = torch.zeros(n_rays, dtype=dtype)
    if vb["type"] != "empty":
        pi = vb["pack_infos_collect"]
        seg = torch.repeat_interleave(torch.arange(pi.shape[0]), pi[:, 1])
        per = torch.zeros(pi.shape[0], dtype=dtype).index_add(0, seg, vb["vw_in_total"].to(dtype).reshape(-1))
        mask = mask.index_put((vb["rays_inds_collect"],), per)
    return mask


def mask_entropy(mode, dtype, *, mask_pred=None, mask_cr=None, mask_dv=None, eps=1.0e-5, w=1.0):
    """the branches of forward_code_single, written out as the reference writes them"""
    p, cr, dv = mask_pred, mask_cr, mask_dv
    lg = lambda x: torch.log(x.clamp_min(eps))                 # noqa: E731
    ent = lambda m: -(m * lg(m) + (1 - m) * lg(1 - m)).mean()  # noqa: E731
    if mode == "nop":
        return {}
    if mode == "cross_cr_on_dv":
        return {"loss_mask_entropy.cross_cr_on_dv": w * (cr * lg(dv)).mean()}
    if mode == "cross_cr_detached_on_dv":
        return {"loss_mask_entropy.cross_cr_on_dv": w * (cr.detach() * lg(dv)).mean()}
    if mode == "cross_dv_on_cr":
        return {"loss_mask_entropy.cross_dv_on_cr": w * (dv * lg(cr)).mean()}
    if mode == "cross_dv_detached_on_cr":
        return {"loss_mask_entropy.cross_dv_on_cr": w * (dv.detach() * lg(cr)).mean()}
    if mode == "cross_crdv":
        return {"loss_mask_entropy.cross_cr_on_dv": w * (cr * lg(dv)).mean(), "loss_mask_entropy.cross_dv_on_cr": w * (dv * lg(cr)).mean()}
    if mode == "cross_crdv_detached":
        return {"loss_mask_entropy.cross_cr_on_dv": w * (cr.detach() * lg(dv)).mean(),
                "loss_mask_entropy.cross_dv_on_cr": w * (dv.detach() * lg(cr)).mean()}
    full = lambda a, b: (a * lg(b.detach()) + (1 - a) * lg(1 - b.detach())).mean()     # noqa: E731
    if mode == "cross_cr_on_dv_detached_full":
        return {"loss_mask_entropy.cross_cr_on_cr": w * full(cr, dv)}
    if mode == "cross_dv_on_cr_detached_full":
        return {"loss_mask_entropy.cross_cr_on_dv": w * full(dv, cr)}
    if mode == "cross_crdv_detached_full":
        return {"loss_mask_entropy.cross_crdv.1": w * full(cr, dv), "loss_mask_entropy.cross_crdv.2": w * full(dv, cr)}
    if mode == "crisp_cr":
        return {"loss_mask_entropy.crisp_cr": w * ent(cr)}
    if mode == "crisp_cr_0":
        return {"loss_mask_entropy.crisp_cr": w * -((1 - cr) * lg(1 - cr)).mean()}
    if mode == "crisp_cr_1":
        return {"loss_mask_entropy.crisp_cr": w * -(cr * lg(cr)).mean()}
    if mode == "crisp_dv":
        return {"loss_mask_entropy.crisp_dv": w * ent(dv)}
    if mode == "crisp_crdv":
        return {"loss_mask_entropy.crisp_cr": w * ent(cr), "loss_mask_entropy.crisp_dv": w * ent(dv)}
    if mode == "crisp_cr_1_dv_0":
        return {"loss_mask_entropy.crisp_cr": w * -(cr * lg(cr)).mean(), "loss_mask_entropy.crisp_dv": w * -((1 - dv) * lg(1 - dv)).mean()}
    if mode == "crisp_cr_0_dv_1":
        return {"loss_mask_entropy.crisp_cr": w * -((1 - cr) * lg(1 - cr)).mean(), "loss_mask_entropy.crisp_dv": w * -(dv * lg(dv)).mean()}
    if mode == "crisp_cr_and_cross_cr_detached_on_dv":          # (the reference reports these two unweighted)
        return {"loss_mask_entropy.crisp_cr": ent(cr), "loss_mask_entropy.cross_cr_on_dv": (cr.detach() * lg(dv)).mean()}
    if mode == "crisp":
        return {"loss_mask_entropy": w * ent(p)}
    raise RuntimeError(f"Invalid mode={mode}")


ENTROPY_MODES = ["crisp", "crisp_cr", "crisp_cr_0", "crisp_cr_1", "crisp_dv", "crisp_crdv", "crisp_cr_1_dv_0", "crisp_cr_0_dv_1",
                 "cross_cr_on_dv", "cross_cr_detached_on_dv", "cross_dv_on_cr", "cross_dv_detached_on_cr", "cross_crdv",
                 "cross_crdv_detached", "cross_cr_on_dv_detached_full", "cross_dv_on_cr_detached_full", "cross_crdv_detached_full",
                 "crisp_cr_and_cross_cr_detached_on_dv", "nop"]


# ------------------------------------------------------------------------------------------------ sparsity / clearance
def sparsity(x, type="normalized_logistic_density", w=1.0, **param):
    if type == "normalized_logistic_density":
        s = torch.sigmoid(x * param.get("inv_scale", 16.0))
        return w * (4.0 * s * (1.0 - s)).mean()
    if type == "normal":
        return w * torch.exp(-x ** param.get("std", 1.0)).mean()
    if type == "density_reg":
        return w * (1 - (-param.get("lamb", 0.05) * x).exp()).abs().mean()
    raise RuntimeError(f"Invalid type={type}")


def clearance(near_sdf, below, beta=1.0, thresh=0.01, w=1.0):
    """``below``: near_sdf < thresh, decided on the float32 inputs"""
    if not bool(below.any()):
        return w * (near_sdf * 0.0).sum()
    return w * torch.exp(-beta * (near_sdf[below] - thresh)).sum() / below.numel()


# ------------------------------------------------------------------------------------------------ lidar
def lidar_valid(depth32, mask32, ranges32, *, discard_toofar=None, mask_pred_thresh=1.0e-7, toofar_replaces_mask=False):
    """-> (valid, err) on the float32 inputs, as float32 (lidar.py:264-266, 280)"""
    valid = (mask32 > mask_pred_thresh) & (ranges32 > 0)
    if discard_toofar is not None and discard_toofar > 0:
        gate = ranges32 <= discard_toofar
        valid = gate if toofar_replaces_mask else (valid & gate)
    return valid, (depth32 - ranges32).abs() * valid.float()


def lidar_keep(valid, err32, factor):
    """-> (keep, median, threshold): the median gate of lidar.py:277-284, the product formed in float32"""
    if not (factor and factor > 0):
        return valid.clone(), None, None
    median = torch.sort(err32).values[err32.numel() // 2]
    thr = median * factor
    return valid & ~(err32 > thr), median, thr


def los_membership(t32, ranges32, vb, fn_type, bound):
    """member [S] on the float32 inputs: 1 neighbor, 2 empty, 0 neither; and the ray of every sample"""
    rih, pi = vb["rays_inds_hit"], vb["pack_infos_hit"]
    seg = torch.repeat_interleave(torch.arange(pi.shape[0]), pi[:, 1])
    g = ranges32[rih][seg]
    b = torch.tensor(bound, dtype=torch.float32)
    member = torch.zeros(t32.shape[0], dtype=torch.uint8)
    if fn_type in ("nerf", "neus_urban"):
        member[(t32 <= g + b) & (t32 >= g - b)] = 1
        member[t32 < g - b] = 2
    else:
        member[(t32 - g).abs() > b] = 2
    return member, seg


def depth_fn(pred, gt, fn_type, far=None, alpha=1.0):
    if fn_type == "l1":
        return (pred - gt).abs()
    if fn_type == "l1_log":
        return (torch.log(pred + 1) - torch.log(gt + 1)).abs()
    if fn_type == "l2":
        return (pred - gt) ** 2
    if fn_type == "l2_relative":
        return (pred - gt) ** 2 / (gt ** 2 + 1e-2)
    if fn_type == "l2_normalized":
        return (pred / far - gt / far) ** 2
    if fn_type == "huber":
        return F.huber_loss(pred, gt, reduction="none", delta=alpha)
    raise ValueError(fn_type)


def lidar(depth, vw, dtype, depth32, mask32, ranges32, vb, *, depth_cfg=None, los_cfg=None, discard_toofar=None,
          discard_outliers_median=100.0, mask_pred_thresh=1.0e-7, far=None, it=0, toofar_replaces_mask=False):
    """-> (losses dict, info dict(valid, keep, member, median, epsilon)).  ``depth`` / ``vw``: leaves of ``dtype`` holding the values
    of depth32 / vb['vw']; every discrete decision is taken on the float32 tensors."""
    valid, err32 = lidar_valid(depth32, mask32, ranges32, discard_toofar=discard_toofar, mask_pred_thresh=mask_pred_thresh,
                               toofar_replaces_mask=toofar_replaces_mask)
    keep, median, thr = lidar_keep(valid, err32, discard_outliers_median)
    out, info = {}, dict(valid=valid, keep=keep, median=median, err=err32, thr=thr, member=None)
    g = ranges32.to(dtype)
    m = keep.to(dtype)
    if depth_cfg is not None:
        w = depth_cfg.get("w", 1.0) if depth_cfg.get("anneal") is None else get_anneal_val(**depth_cfg["anneal"], it=it)
        fp = depth_cfg.get("fn_param") or {}
        out["lidar_loss.depth"] = w * (depth_fn(depth, g, depth_cfg.get("fn_type", "l1_log"), far=far, alpha=fp.get("alpha", 1.0)) * m).mean()
    if los_cfg is not None and vb["type"] != "empty":
        w = los_cfg.get("w", 1.0) if los_cfg.get("anneal") is None else get_anneal_val(**los_cfg["anneal"], it=it)
        fn_type, fp = los_cfg.get("fn_type", "nerf"), los_cfg.get("fn_param") or {}
        t32 = vb["t"].float()
        if fn_type in ("nerf", "neus_urban"):
            bound = fp.get("sigma", 1.0)
            std = bound / fp.get("sigma_scale_factor", 3.0)
        else:
            bound = fp.get("epsilon", 1.0) if fp.get("epsilon_anneal") is None else get_anneal_val(**fp["epsilon_anneal"], it=it)
        member, seg = los_membership(t32, ranges32, vb, fn_type, bound)
        info.update(member=member, epsilon=bound)
        R = vb["rays_inds_hit"].shape[0]
        m_hit = m[vb["rays_inds_hit"]]
        ray_sum = lambda x: torch.zeros(R, dtype=dtype).index_add(0, seg, x)      # noqa: E731
        if fn_type in ("nerf", "neus_urban"):
            d = t32.to(dtype) - g[vb["rays_inds_hit"]][seg]
            dens = torch.exp(-0.5 * (d / std) ** 2) / (std * math.sqrt(2.0 * math.pi))
            out["lidar_loss.los.neighbor"] = w * (ray_sum((member == 1).to(dtype) * (vw - dens) ** 2) * m_hit).mean()
        out["lidar_loss.los.empty"] = w * (ray_sum((member == 2).to(dtype) * vw ** 2) * m_hit).mean()
    return out, info
