"""The monocular depth / normal cue losses (neuralsim_amd/losses.py: ``mono_remain_mask``, ``mono_depth_ssi_loss``,
``mono_depth_pearson_loss``, ``mono_normal_cue_loss``, ``packed_share``; kernels in csrc/loss_ops.hip) at the configs' patch sizes
64x64 and 80x120 and on a 320x480 quarter-resolution image.

1. Every op, forward + backward, beside the same formula as a composition of torch ops on the device (the formulas of
   app/loss/mono.py; the erosion as a max-pool of the complement, ``packed_sum`` as an ``index_add``), both on the same inputs in one
   process, hip and torch ALTERNATED in blocks of 5.  Per variant: the median and the 10 / 90 % points of the HIP events and of
   the host clock around a synchronised forward + backward, after ``--warmup`` pairs; C-ABI calls and ATen operator calls of
   the forward and of the backward.
2. The small indoor step three ways, alternated: ``hip`` (``INDOOR_MONO_LOSS_CFG`` on the ops), ``torch`` (the same trainer, the ops
   replaced by the compositions of this file) and ``none`` (no ``loss_cfg`` and no ``mono`` terms, on the same autograd path).

Prints one JSON line.

    python tools/mono_loss_bench.py [--repeats 40] [--warmup 10] [--out profiles/mono_loss_bench.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


# ------------------------------------------------------------------------------------------------ the torch compositions
def t_remain(mask_pred, depth0, depth, gt, occ, human, far, thresh, erode):
    """the street yaml's list (pred_not_occupied, human, not_occupied) + toofar, eroded"""
    import torch.nn.functional as F
    ign = ~(mask_pred > thresh) | human | ~occ | (depth0 > far)
    if erode > 0:
        x = F.pad(ign.float()[None, None], (erode, erode - 1, erode, erode - 1))
        ign = F.max_pool2d(x, 2 * erode, 1)[0, 0] > 0
    return ~ign


def t_ssi(pred, gt, mask, *, fn_type="mse", gt_pre_scale=1.0, gt_pre_shift=0.0, alpha_grad_reg=0.01, grad_reg_scales=4, w=1.0):
    import torch
    target = gt_pre_scale * gt + gt_pre_shift
    m = mask.float()
    a00, a01, a11 = (m * pred * pred).sum(), (m * pred).sum(), m.sum()
    b0, b1 = (m * pred * target).sum(), (m * target).sum()
    det = a00 * a11 - a01 * a01
    ok = det != 0                     # (the reference reads det.item(); kept on the device here, in the composition's favour)
    safe = torch.where(ok, det, torch.ones_like(det))
    scale = torch.where(ok, (a11 * b0 - a01 * b1) / safe, torch.zeros_like(det))
    shift = torch.where(ok, (-a01 * b0 + a00 * b1) / safe, torch.zeros_like(det))
    p = scale * pred + shift
    d = p - target
    loss = w * ((d * d if fn_type == "mse" else d.abs()) * m).mean()
    reg = 0
    for k in range(grad_reg_scales):
        s = 2 ** k
        df, mk = (d * m)[::s, ::s], mask[::s, ::s]
        reg = reg + ((mk[:, 1:] & mk[:, :-1]) * (df[:, 1:] - df[:, :-1]).abs()).sum() \
            + ((mk[1:, :] & mk[:-1, :]) * (df[1:, :] - df[:-1, :]).abs()).sum()
    return loss, w * alpha_grad_reg * reg


def _pearson(a, b):
    a, b = a - a.mean(), b - b.mean()
    return (a * b).sum() / (a.norm() * b.norm()).clamp_min(1e-12)


def t_pearson(pred, gt, mask, alpha_grad_reg=0.01, grad_reg_scales=4, w=1.0):
    reg = 0
    for k in range(grad_reg_scales):
        s = 2 ** k
        p, g, m = pred[::s, ::s], gt[::s, ::s], mask[::s, ::s]
        mx, my = m[:, 1:] & m[:, :-1], m[1:, :] & m[:-1, :]
        if mx.any():                  # the reference's host read
            reg = reg + 1 - _pearson((p[:, 1:] - p[:, :-1])[mx], (g[:, 1:] - g[:, :-1])[mx])
        if my.any():
            reg = reg + 1 - _pearson((p[1:, :] - p[:-1, :])[my], (g[1:, :] - g[:-1, :])[my])
    return w * (1 - _pearson(pred[mask], gt[mask])), w * alpha_grad_reg * reg


def t_normals(n_pred, n_gt, mask, rot, w_l1=1.0, w_cos=1.0):
    import torch.nn.functional as F
    n = (rot * n_pred.unsqueeze(-2)).sum(-1)
    a, b = F.normalize(n, dim=-1), F.normalize(n_gt, dim=-1)
    m = mask.float()
    return w_l1 * ((a - b).abs().sum(-1) * m).mean(), w_cos * ((1 - (a * b).sum(-1)) * m).mean()


def t_share(vw, t, rgb, seg, rays_inds, N):
    import torch
    P = rays_inds.shape[0]
    dev = vw.device
    m = torch.zeros(P, device=dev).index_add(0, seg, vw)
    d = torch.zeros(P, device=dev).index_add(0, seg, vw * t)
    c = torch.zeros(P, 3, device=dev).index_add(0, seg, vw[:, None] * rgb)
    mask = torch.zeros(N, device=dev).index_put((rays_inds,), m)
    depth = torch.zeros(N, device=dev).index_put((rays_inds,), d) / (mask + 1e-10)
    return mask, depth, torch.zeros(N, 3, device=dev).index_put((rays_inds,), c)


def cases(H, W, dev, L):
    """-> (sizes, {op: (the op, its torch composition, the leaves both differentiate)}) on one set of inputs: a coherent scene -- a
    sky band the model does not occupy, a rectangle of people, depths within far -- so that the eroded mask keeps most of the patch"""
    import torch
    g = torch.Generator(device=dev).manual_seed(H * W)
    rnd = lambda *s: torch.rand(*s, device=dev, generator=g)          # noqa: E731
    rows = torch.arange(H, device=dev)[:, None].expand(H, W)
    cols = torch.arange(W, device=dev)[None, :].expand(H, W)
    pred = (rnd(H, W) * 5 + 0.5).requires_grad_(True)
    gt = 0.3 * pred.detach() + 0.1 + 0.05 * (rnd(H, W) - 0.5)
    mask_pred = torch.where(rows < H // 5, 0.1 + 0.2 * rnd(H, W), 0.97 + 0.03 * rnd(H, W))
    occ = rows >= H // 6
    human = (rows >= H // 2) & (rows < H // 2 + H // 8) & (cols >= W // 3) & (cols < W // 3 + W // 10)
    far, thresh, e = 50.0, 0.5, 8
    names = ["pred_not_occupied", "human", "not_occupied", "toofar"]
    d0 = pred.detach()
    remain = t_remain(mask_pred, d0, d0, gt, occ, human, far, thresh, e)
    mine = L.mono_remain_mask(mask_pred, depth_pred0=d0, occupancy_gt=occ, human_gt=human, far=far, ignore_mask_list=names,
                              mask_pred_thresh=thresh, mask_erode=e)
    assert torch.equal(mine, remain), "the two remain masks differ"
    assert int(remain.sum()) > H * W // 4
    N = H * W
    n_pred, n_gt = torch.randn(N, 3, device=dev, generator=g).requires_grad_(True), torch.randn(N, 3, device=dev, generator=g)
    rot = torch.linalg.qr(torch.randn(N, 3, 3, device=dev, generator=g))[0].contiguous()
    K = 24                                   # samples per ray of the object's buffer; every second ray is hit
    hit = torch.arange(0, N, 2, device=dev)
    P = hit.shape[0]
    pi = torch.stack([torch.arange(P, device=dev) * K, torch.full([P], K, device=dev)], 1)
    seg = torch.arange(P, device=dev).repeat_interleave(K)
    vw, tt = (rnd(P * K) / K).requires_grad_(True), rnd(P * K) * 6
    rgb = rnd(P * K, 3).requires_grad_(True)
    kw = dict(gt_pre_scale=50.0, gt_pre_shift=1.0, alpha_grad_reg=0.01, grad_reg_scales=4, w=1.0e-3)
    flat = remain.reshape(-1)
    cs = dict(
        remain_mask=(lambda: (L.mono_remain_mask(mask_pred, depth_pred0=d0, occupancy_gt=occ, human_gt=human, far=far, ignore_mask_list=names,
                                                 mask_pred_thresh=thresh, mask_erode=e),),
                     lambda: (t_remain(mask_pred, d0, d0, gt, occ, human, far, thresh, e),), []),
        ssi_depth_mse=(lambda p: L.mono_depth_ssi_loss(p, gt, remain, fn_type="mse", **kw), lambda p: t_ssi(p, gt, remain, fn_type="mse", **kw), [pred]),
        ssi_depth_l1=(lambda p: L.mono_depth_ssi_loss(p, gt, remain, fn_type="l1", **kw), lambda p: t_ssi(p, gt, remain, fn_type="l1", **kw), [pred]),
        pearson_depth=(lambda p: L.mono_depth_pearson_loss(p, gt, remain), lambda p: t_pearson(p, gt, remain), [pred]),
        normal_cue=(lambda n: L.mono_normal_cue_loss(n, n_gt, flat, rot=rot, w_l1=0.01, w_cos=0.01),
                    lambda n: t_normals(n, n_gt, flat, rot, 0.01, 0.01), [n_pred]),
        packed_share=(lambda v, c: L.packed_share(v, tt, c, None, pi, hit, N), lambda v, c: t_share(v, tt, c, seg, hit, N), [vw, rgb]),
    )
    return dict(remaining_pixels=int(remain.sum()), share_samples=P * K), cs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step-blocks", type=int, default=6)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode
    from neuralsim_amd import _lib, losses as L, scenarios as sc
    assert torch.cuda.is_available(), "mono_loss_bench measures on the device"
    dev = torch.device("cuda", 0)

    class Count(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, a=(), kw=None):
            Count.n += 1
            return func(*a, **(kw or {}))

    def med(xs):
        xs = sorted(xs)
        q = lambda f: round(xs[min(len(xs) - 1, int(f * len(xs)))], 5)          # noqa: E731
        return dict(p50=q(0.5), p10=q(0.1), p90=q(0.9))

    def pair(fwd, leaves):
        """forward + backward of sum of the terms, gradients cleared"""
        def run(count=None):
            for x in leaves:
                x.grad = None
            if count is not None:
                Count.n, _lib.CALL_COUNT = 0, 0
            tot = sum(v.sum() for v in fwd(*leaves) if v is not None and v.is_floating_point())
            if count is not None:
                count["fwd"] = dict(c_abi_calls=_lib.CALL_COUNT, aten_ops=Count.n)
                Count.n, _lib.CALL_COUNT = 0, 0
            if torch.is_tensor(tot) and tot.requires_grad:
                tot.backward()
            if count is not None:
                count["bwd"] = dict(c_abi_calls=_lib.CALL_COUNT, aten_ops=Count.n)
        return run

    def timed(p):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        p()
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)

    def measure(pairs):
        for p in pairs.values():
            for _ in range(args.warmup):
                p()
        torch.cuda.synchronize()
        host, evs = {k: [] for k in pairs}, {k: [] for k in pairs}
        for _ in range(max(4, args.repeats // 5)):
            for k, p in pairs.items():
                for _ in range(5):
                    h, e = timed(p)
                    host[k].append(h)
                    evs[k].append(e)
        res = {}
        for k, p in pairs.items():
            cnt = {}
            with Count():
                p(cnt)
            _lib.CALL_COUNT = None
            torch.cuda.synchronize()
            res[k] = dict(gpu_events_ms=med(evs[k]), host_ms=med(host[k]), repeats=len(evs[k]), launches=cnt)
        res["ratio_torch_over_hip"] = dict(gpu_events=round(res["torch"]["gpu_events_ms"]["p50"] / res["hip"]["gpu_events_ms"]["p50"], 3),
                                           host=round(res["torch"]["host_ms"]["p50"] / res["hip"]["host_ms"]["p50"], 3))
        res["hip_ahead_by_more_than_the_spread"] = res["torch"]["gpu_events_ms"]["p10"] > res["hip"]["gpu_events_ms"]["p90"]
        return res

    out = dict(tool="mono_loss_bench", device=torch.cuda.get_device_name(0), torch=torch.__version__, repeats=args.repeats,
               warmup=args.warmup, sizes={})
    for H, W in ((64, 64), (80, 120), (320, 480)):
        info, cs = cases(H, W, dev, L)
        res = {name: measure(dict(hip=pair(hip, leaves), torch=pair(tor, leaves))) for name, (hip, tor, leaves) in cs.items()}
        out["sizes"][f"{H}x{W}"] = dict(**info, **res)

    # ---- the small indoor step: with the ops / with the compositions / without the terms
    def t_depth_block(pred, gt, mask, **kw):
        kw.pop("detach_scale_shift", None), kw.pop("scale_gt_to_pred", None)
        return t_ssi(pred, gt, mask, **kw)

    def build(mode):
        torch.manual_seed(0)
        cfg = None if mode == "none" else dict(sc.INDOOR_MONO_LOSS_CFG, mono_depth=dict(sc.INDOOR_MONO_LOSS_CFG["mono_depth"], enable_after=0))
        tr = sc.build_indoor_trainer(dev, small=True, rays_per_gpu=1024, loss_cfg=cfg)
        if mode == "none":
            tr.mono, tr.fused_step = None, False       # the same autograd-path step, minus the terms
        return tr
    trainers = {m: build(m) for m in ("hip", "torch", "none")}
    real = (L.mono_depth_ssi_loss, L.mono_normal_cue_loss, L.mono_remain_mask)

    def swap(on):
        if on:
            L.mono_depth_ssi_loss = t_depth_block
            L.mono_normal_cue_loss = lambda a, b, m, rot=None, w_l1=1.0, w_cos=1.0: t_normals(a, b, m, torch.eye(3, device=dev), w_l1, w_cos)
            L.mono_remain_mask = lambda mp, **k: torch.ones_like(mp, dtype=torch.bool)      # the yaml's empty lists: every pixel
        else:
            L.mono_depth_ssi_loss, L.mono_normal_cue_loss, L.mono_remain_mask = real
    times, calls = {m: [] for m in trainers}, {}
    it = {m: 0 for m in trainers}
    for blk in range(args.step_blocks + 1):
        for m, tr in trainers.items():
            swap(m == "torch")
            torch.cuda.synchronize()
            _lib.CALL_COUNT = 0
            t0 = time.perf_counter()
            for _ in range(args.block):
                tr.train_step(it[m])
                it[m] += 1
            torch.cuda.synchronize()
            if blk:                                # the first block warms up
                times[m].append((time.perf_counter() - t0) * 1e3 / args.block)
            calls[m], _lib.CALL_COUNT = _lib.CALL_COUNT / args.block, None
            swap(False)
    out["indoor_small_step"] = dict(rays=1024, patch=list(trainers["hip"].mono["patch_hw"]), blocks=args.step_blocks, block=args.block,
                                    **{m: dict(ms_per_step=med(times[m]), c_abi_calls_per_step=calls[m]) for m in trainers})
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
