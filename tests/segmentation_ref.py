"""Checker of the segmentation z-buffer (``nsim_seg_zbuffer``): the reference's per-group update
(app/renderers/buffer_compose_renderer.py:288-309, 439-450, 561-572) restated sequentially on the CPU -- sources in processing
order, each source's candidates in list order; a candidate takes the ray when ``mask > thr`` and ``depth < z[ray]`` (both
strict, in float32 as the tensors are).  Integer and compare logic only: results are compared exactly."""
import math

import numpy as np
import torch


def seg_zbuffer_ref(sources, N: int, thr: float):
    """``sources``: as ``pack_ops.seg_zbuffer`` takes them (pair form, ``bidx`` image form or ``image=True``), on any device.
    -> (ins_seg [N] long, class_seg [N] long, z [N] f32) on the CPU."""
    ins_seg = np.full([N], -1, dtype=np.int64)
    cls_seg = np.full([N], -1, dtype=np.int64)
    z = np.full([N], np.inf, dtype=np.float32)
    thr32 = np.float32(thr)
    for s in sources:
        ri = s["rays_inds"].detach().cpu().long().numpy()
        mask = s["mask"].detach().cpu().float().numpy()
        depth = s["depth"].detach().cpu().float().numpy()
        if s.get("bidx") is not None:
            b = s["bidx"].detach().cpu().long().numpy()
            mask, depth = mask[b, ri], depth[b, ri]
        elif s.get("image", False):
            mask, depth = mask[ri], depth[ri]
        ins = s["ins"]
        ins = ins.detach().cpu().long().numpy() if torch.is_tensor(ins) else np.full(ri.shape, int(ins), dtype=np.int64)
        for j in range(ri.shape[0]):
            r = int(ri[j])
            if mask[j] > thr32 and depth[j] < z[r]:          # (a NaN compares false both times)
                z[r] = depth[j]
                ins_seg[r] = ins[j]
                cls_seg[r] = int(s["class_ind"])
    return torch.from_numpy(ins_seg), torch.from_numpy(cls_seg), torch.from_numpy(z)


def ambiguous_rays(per_obj, thr: float, mask_tol: float, depth_tol: float):
    """Rays whose segmentation two runs with slightly different arithmetic may decide differently: some object's individual
    mask lies within ``mask_tol`` of the threshold, or the two nearest qualifying depths differ by less than ``depth_tol``.
    ``per_obj``: id -> dict(mask_volume [N], depth_volume [N]).  -> bool [N]."""
    masks = torch.stack([v["mask_volume"].detach().cpu().float() for v in per_obj.values()])        # [O, N]
    depths = torch.stack([v["depth_volume"].detach().cpu().float() for v in per_obj.values()])
    near_thr = ((masks - thr).abs() <= mask_tol).any(0)
    d = torch.where(masks > thr, depths, torch.full_like(depths, math.inf))
    if d.shape[0] < 2:
        return near_thr
    two = torch.topk(d, 2, dim=0, largest=False).values
    close = torch.isfinite(two[1]) & ((two[1] - two[0]) < depth_tol)
    return near_thr | close
