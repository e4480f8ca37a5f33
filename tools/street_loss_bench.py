"""The street configs' supervision losses (neuralsim_amd/losses.py: ``mask_occupancy_loss``, ``mask_entropy_loss``, ``sparsity_loss``,
``clearance_loss``, ``kth_value``, ``lidar_loss``; kernels in csrc/loss_ops.hip) at the street sizes: 8192 pixel rays, 8192 beams,
and the sample counts a street step of ``build_street_trainer`` produces.

1. Every op, forward + backward, on tensors captured from one street iteration, beside the same formula as a composition of torch
   ops on the device (``torch.sort`` for the median of the lidar loss, ``.item()`` for the clearance count, as the reference's
   classes have them).  Per variant: the median and the 10 / 90 % points of the host clock around a synchronised pair and of the HIP
   events around it, after ``--warmup`` pairs; C-ABI calls and ATen operator calls of one pair; hip and torch ALTERNATED in blocks.
2. The street iteration (pixel + lidar step) three ways, alternated ``--rounds`` times in one process: ``hip`` (the yaml's
   ``loss_cfg`` on the new ops), ``torch`` (the same trainer, the ops replaced by the torch compositions of this file) and
   ``none`` (no ``loss_cfg``: the step as it was).  Blocks of ``--block`` iterations with one synchronisation at the end of a block;
   C-ABI calls per iteration beside each.

Prints one JSON line.

    python tools/street_loss_bench.py [--repeats 40] [--warmup 10] [--out profiles/street_loss_bench.json]
"""
import argparse
import contextlib
import json
import math
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


# ------------------------------------------------------------------------------------------------ the torch compositions
def t_mask(pred, gt, *, pred_clip=1e-3, safe_bce=True, bce_limit=0.1, special_mask_mode=None, w=1.0):
    import torch.nn.functional as F
    p = pred.clip(pred_clip, 1.0 - pred_clip) if (pred_clip is not None and pred_clip > 0) or not safe_bce else pred
    if safe_bce:
        p = p.clamp(bce_limit, 1.0 - bce_limit)
    assert special_mask_mode is None
    return w * F.binary_cross_entropy(p, gt), (pred.detach() - gt).abs()


def t_object_mask(vb, n, device=None):
    import torch
    from neuralsim_amd.graphics import pack_ops as po
    m = torch.zeros(n, device=device if vb["type"] == "empty" else vb["vw_in_total"].device)
    if vb["type"] != "empty":
        m = m.index_put((vb["rays_inds_collect"],), po.packed_sum(vb["vw_in_total"].reshape(-1), vb["pack_infos_collect"]))
    return m


def t_entropy(mode, *, mask_pred=None, mask_cr=None, mask_dv=None, eps=1e-5, w=1.0):
    import torch
    assert mode == "crisp_cr"
    m = mask_cr
    return {"loss_mask_entropy.crisp_cr": w * -(m * torch.log(m.clamp_min(eps)) + (1 - m) * torch.log((1 - m).clamp_min(eps))).mean()}


def t_sparsity(x, type="normalized_logistic_density", inv_scale=16.0, w=1.0):
    import torch
    s = torch.sigmoid(x * inv_scale)
    return w * (4.0 * s * (1.0 - s)).mean()


def t_clearance(near_sdf, beta=1.0, thresh=0.01, w=1.0):
    import torch
    inside = near_sdf < thresh
    if inside.sum().item() == 0:                    # the reference's host read (clearance.py:53)
        return w * near_sdf.new_zeros([])
    return w * torch.exp(-beta * (near_sdf[inside] - thresh)).sum() / inside.numel()


def t_lidar(rendered, vb, ranges, *, depth=None, line_of_sight=None, discard_toofar=None, discard_outliers=0,
            discard_outliers_median=100.0, mask_pred_thresh=1e-7, far=None, it=0, toofar_replaces_mask=False, aux=None):
    import torch
    from neuralsim_amd.graphics import pack_ops as po
    from nr3d_lib.models.annealers import get_anneal_val
    d, m = rendered["depth_volume"], rendered["mask_volume"]
    mask = (m.detach() > mask_pred_thresh) & (ranges > 0)
    if discard_toofar:
        mask = mask & (ranges <= discard_toofar)
    with torch.no_grad():
        err = (d - ranges).abs() * mask
        median = torch.sort(err).values[d.numel() // 2]             # the full sort of lidar.py:281
        mask = mask & ~(err > median * discard_outliers_median)
    mf = mask.float()
    out = {"lidar_loss.depth": depth["w"] * ((d - ranges).abs() * mf).mean()}
    if vb["type"] != "empty":
        fp = line_of_sight["fn_param"]
        eps = get_anneal_val(**fp["epsilon_anneal"], it=it) if fp.get("epsilon_anneal") else fp.get("epsilon", 1.0)
        rih, pi = vb["rays_inds_hit"], vb["pack_infos_hit"]
        gt_ex = torch.repeat_interleave(ranges[rih], pi[:, 1], dim=0)
        empty = po.packed_sum(((vb["t"] - gt_ex).abs() > eps) * vb["vw"] ** 2, pi).reshape(-1)
        out["lidar_loss.los.empty"] = line_of_sight["w"] * (empty * mf[rih]).mean()
    return out


TORCH_OPS = dict(mask_occupancy_loss=t_mask, object_mask_in_total=t_object_mask, mask_entropy_loss=t_entropy, sparsity_loss=t_sparsity,
                 clearance_loss=t_clearance, lidar_loss=t_lidar)


@contextlib.contextmanager
def torch_ops(losses):
    """``neuralsim_amd.losses`` with the street ops replaced by the compositions above (the trainer looks them up per step)"""
    saved = {k: getattr(losses, k) for k in TORCH_OPS}
    for k, v in TORCH_OPS.items():
        setattr(losses, k, v)
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(losses, k, v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--it", type=int, default=3000, help="iteration the schedules are evaluated at (all blocks enabled)")
    ap.add_argument("--no-step", action="store_true", help="skip part 2")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import copy
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode
    from neuralsim_amd import _lib, losses, scenarios as sc
    assert torch.cuda.is_available(), "street_loss_bench needs a HIP device"
    dev = torch.device("cuda", 0)

    class Count(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            Count.n += 1
            return func(*args, **(kwargs or {}))

    def med(ts):
        ts = sorted(ts)
        return dict(p50=round(ts[len(ts) // 2], 5), p10=round(ts[len(ts) // 10], 5), p90=round(ts[(9 * len(ts)) // 10], 5))

    def timed(pair):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        pair()
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)

    def measure(pairs):
        """pairs: {variant: callable}; alternated in blocks of 5"""
        for p in pairs.values():
            for _ in range(args.warmup):
                p()
        torch.cuda.synchronize()
        host, evs = {k: [] for k in pairs}, {k: [] for k in pairs}
        for _ in range(max(1, args.repeats // 5)):
            for k, p in pairs.items():
                for _ in range(5):
                    h, e = timed(p)
                    host[k].append(h)
                    evs[k].append(e)
        res = {}
        for k, p in pairs.items():
            Count.n, _lib.CALL_COUNT = 0, 0
            with Count():
                p()
            calls, _lib.CALL_COUNT = _lib.CALL_COUNT, None
            torch.cuda.synchronize()
            res[k] = dict(host_ms=med(host[k]), gpu_events_ms=med(evs[k]), c_abi_calls=calls, aten_ops=Count.n)
        res["ratio_torch_over_hip"] = dict(host=round(res["torch"]["host_ms"]["p50"] / res["hip"]["host_ms"]["p50"], 3),
                                           gpu_events=round(res["torch"]["gpu_events_ms"]["p50"] / res["hip"]["gpu_events_ms"]["p50"], 3))
        # "beats by more than the spread": the torch p10 lies above the hip p90
        res["hip_ahead_by_more_than_the_spread"] = dict(host=res["torch"]["host_ms"]["p10"] > res["hip"]["host_ms"]["p90"],
                                                         gpu_events=res["torch"]["gpu_events_ms"]["p10"] > res["hip"]["gpu_events_ms"]["p90"])
        return res

    cfg = copy.deepcopy(sc.STREET_LOSS_CFG)
    out = dict(tool="street_loss_bench", rays=args.rays, beams=args.rays, it=args.it, repeats=args.repeats, warmup=args.warmup,
               device=torch.cuda.get_device_name(0))
    # ---- tensors of one real street iteration
    torch.manual_seed(0)
    tr = sc.build_street_trainer(dev, 0, 1, rays_per_gpu=args.rays, lidar_rays=args.rays, loss_cfg=cfg)
    seen = {}
    loss0, render0, sample0 = tr.loss, tr.renderer.render, tr.sample_lidar_batch

    def spy_loss(ret, gt, uni=None, aux=None):
        seen["pixel"] = (ret, aux)
        return loss0(ret, gt, uni, aux=aux)

    def spy_render(*a, **k):
        seen["ret"] = render0(*a, **k)
        return seen["ret"]

    def spy_sample():
        seen["beams"] = sample0()
        return seen["beams"]
    tr.loss, tr.renderer.render, tr.sample_lidar_batch = spy_loss, spy_render, spy_sample
    for i in range(3):
        tr.train_step(args.it + i)
    torch.cuda.synchronize()
    tr.loss, tr.renderer.render, tr.sample_lidar_batch = loss0, render0, sample0
    ret, aux = seen["pixel"]
    lret, ranges = seen["ret"], seen["beams"][2]
    det = lambda x: x.detach().clone()      # noqa: E731
    mask_pred, mask_gt = det(ret["rendered"]["mask_volume"]), det(aux["mask"])
    cr_vb = {k: (det(v) if torch.is_tensor(v) else v) for k, v in ret["raw_per_obj_model"]["main"]["volume_buffer"].items()
             if k in ("type", "vw_in_total", "rays_inds_collect", "pack_infos_collect")}
    sdf, near = det(ret["raw_per_obj_model"]["main"]["extra_pts"]["sdf"]), det(ret["raw_per_obj_model"]["main"]["details"]["near_sdf"])
    vb = {k: (det(v) if torch.is_tensor(v) else v) for k, v in lret["volume_buffer"].items() if k in ("type", "t", "vw", "rays_inds_hit", "pack_infos_hit")}
    depth, lmask, ranges = det(lret["rendered"]["depth_volume"]), det(lret["rendered"]["mask_volume"]), det(ranges)
    N = mask_pred.shape[0]
    out["near_points_below_thresh"] = int((near < 0.02).sum())
    out["sizes"] = dict(pixel_rays=N, beams=int(depth.shape[0]), uniform_points=int(sdf.shape[0]), near_points=int(near.shape[0]),
                        cr_samples_pixel=int(cr_vb["vw_in_total"].shape[0]) if cr_vb["type"] != "empty" else 0,
                        lidar_samples=int(vb["t"].shape[0]), lidar_packs=int(vb["rays_inds_hit"].shape[0]))
    lcfg = {k: v for k, v in cfg["lidar"].items()}
    sp = {k: v for k, v in cfg["sparsity"]["class_name_cfgs"]["Street"].items() if k in ("inv_scale", "w")}

    def leaf(x):
        return x.detach().requires_grad_(True)

    def bw(v):          # (the torch clearance with no point below the threshold is a constant, as the reference's)
        if v.requires_grad:
            v.backward()

    def pair_of(mod):
        """forward + backward of every op through ``mod``'s functions"""
        def mask():
            p = leaf(mask_pred)
            bw(mod["mask_occupancy_loss"](p, mask_gt, safe_bce=True, pred_clip=0, w=0.3)[0])

        def entropy():
            v = leaf(cr_vb["vw_in_total"])
            m = mod["object_mask_in_total"](dict(cr_vb, vw_in_total=v), N)
            bw(mod["mask_entropy_loss"]("crisp_cr", mask_cr=m, w=0.005)["loss_mask_entropy.crisp_cr"])

        def entropy_alone():
            m = leaf(mask_pred)
            bw(mod["mask_entropy_loss"]("crisp_cr", mask_cr=m, w=0.005)["loss_mask_entropy.crisp_cr"])

        def sparsity():
            bw(mod["sparsity_loss"](leaf(sdf), "normalized_logistic_density", **sp))

        def clearance():
            bw(mod["clearance_loss"](leaf(near), beta=10.0, thresh=0.02, w=0.2))

        def lidar():
            d, w_ = leaf(depth), leaf(vb["vw"])
            o = mod["lidar_loss"](dict(depth_volume=d, mask_volume=lmask), dict(vb, vw=w_), ranges, it=args.it, **lcfg)
            bw(sum(o.values()))
        return dict(mask_occupancy=mask, mask_entropy_with_object_mask=entropy, mask_entropy=entropy_alone, sparsity=sparsity,
                    clearance=clearance, lidar=lidar)

    hip = pair_of({k: getattr(losses, k) for k in TORCH_OPS})
    tch = pair_of(TORCH_OPS)
    out["fwd_bwd_pair"] = {name: measure(dict(hip=hip[name], torch=tch[name])) for name in hip}
    x = (depth - ranges).abs()
    out["fwd_bwd_pair"]["median"] = measure(dict(hip=lambda: losses.kth_value(x, x.numel() // 2),
                                                 torch=lambda: torch.sort(x).values[x.numel() // 2]))
    assert int(losses.kth_value(x, x.numel() // 2).view(torch.int32)) == int(torch.sort(x).values[x.numel() // 2].view(torch.int32))
    # agreement of the two variants on the lidar loss (value) -- the tests hold the ops to float64; this guards the tool's formulas
    d_ = dict(depth_volume=depth, mask_volume=lmask)
    a, b = losses.lidar_loss(d_, vb, ranges, it=args.it, **lcfg), t_lidar(d_, vb, ranges, it=args.it, **lcfg)
    out["agreement_lidar"] = {k: float((a[k] - b[k]).abs() / b[k].abs().clamp_min(1e-12)) for k in a}
    del tr
    if not args.no_step:
        trs = {}
        for mode in ("hip", "torch", "none"):
            torch.manual_seed(0)
            trs[mode] = [sc.build_street_trainer(dev, 0, 1, rays_per_gpu=args.rays, lidar_rays=args.rays,
                                                 loss_cfg=None if mode == "none" else copy.deepcopy(cfg)), args.it]

        def ctx(mode):
            return torch_ops(losses) if mode == "torch" else contextlib.nullcontext()
        for m, st in trs.items():
            with ctx(m):
                for _ in range(max(args.warmup, 20)):
                    st[0].train_step(st[1])
                    st[1] += 1
        torch.cuda.synchronize()
        blocks, host, calls = {m: [] for m in trs}, {m: [] for m in trs}, {}
        for _ in range(args.rounds):
            for m, st in trs.items():
                with ctx(m):
                    for _ in range(args.blocks):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(args.block):
                            st[0].train_step(st[1])
                            st[1] += 1
                        t1 = time.perf_counter()
                        torch.cuda.synchronize()
                        blocks[m].append((time.perf_counter() - t0) * 1e3 / args.block)
                        host[m].append((t1 - t0) * 1e3 / args.block)
        for m, st in trs.items():
            with ctx(m):
                _lib.CALL_COUNT = 0
                st[0].train_step(st[1])
                st[1] += 1
                calls[m], _lib.CALL_COUNT = _lib.CALL_COUNT, None
        torch.cuda.synchronize()
        out["street_iteration_ms"] = {m: med(b) for m, b in blocks.items()}
        out["street_iteration_host_ms"] = {m: med(b) for m, b in host.items()}
        out["street_iteration_c_abi_calls"] = calls
        p50 = {m: out["street_iteration_ms"][m]["p50"] for m in trs}
        out["street_iteration_cost_of_the_terms_ms"] = dict(hip=round(p50["hip"] - p50["none"], 4), torch=round(p50["torch"] - p50["none"], 4))
        out["street_iteration_hip_ahead_by_more_than_the_spread"] = \
            out["street_iteration_ms"]["torch"]["p10"] > out["street_iteration_ms"]["hip"]["p90"]
        out["parts_after"] = {k: float(v) for k, v in trs["hip"][0].loss_parts.items()}
        out["lidar_parts_after"] = {k: float(v) for k, v in trs["hip"][0]._lidar_parts.items()}
        assert all(math.isfinite(v) for v in list(out["parts_after"].values()) + list(out["lidar_parts_after"].values()))
    print(json.dumps(out))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
