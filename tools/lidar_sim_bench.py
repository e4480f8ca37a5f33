#!/usr/bin/env python
"""Time the simulated-LiDAR kernels (neuralsim_amd/lidar_sim.py) at the size of a real sensor: a 128-beam x 3600-azimuth grid sweep
(460 800 rays) and a 115 010-pair scan pattern.  Three measurements, each against THE REFERENCE'S TORCH COMPOSITION ON THE SAME
DEVICE (restated in this file), alternated ``--repeat`` times in one process after a warm-up of each; a timed window is ``--iters``
calls between two device synchronisations under the host clock, medians of the per-call times:
  * ``nsim_lidar_raygen``  vs  meshgrid, four sin / cos tensors, three broadcast products, normalize, tile (lidars.py:211-230);
  * the returns compaction (count -> scan -> emit, with the one size read)  vs  the mask and the masked gathers of
    render.py:331-346 (with rgb and ids: seven gathers);
  * one full simulated sweep of the street model of tools/occgrid_bench.py (rays, render without gradients, point cloud) with the
    kernels and with the two torch compositions around the same render.
Also recorded: the bytes each kernel must move (computed from the shapes), the GPU time per entry point (HIP events around each
call, a pass of its own) and from both the achieved bandwidth as a fraction of the 8 TB/s HBM peak.  ASSERTED: both sides give the
same ray order / the same returns.  The times are recorded, not gated.
Usage: python tools/lidar_sim_bench.py [--beams 128] [--azimuths 3600] [--pairs 115010] [--iters 50] [--repeat 5]
                                       [--out profiles/lidar_sim_bench.json] [--emulate]"""
import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
HBM_PEAK = 8.0e12


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _window(fn, iters, dev):
    """ms per call over a window of ``iters`` calls"""
    _sync(dev)
    t0 = time.perf_counter()
    for _ in range(iters):
        r = fn()
    _sync(dev)
    return r, (time.perf_counter() - t0) * 1e3 / iters


def _ab(ours, ref, iters, repeat, dev):
    ours(), ref()                                   # warm-up
    a, b = [], []
    for _ in range(repeat):
        a.append(_window(ours, iters, dev)[1])
        b.append(_window(ref, iters, dev)[1])
    return dict(kernels_ms=round(statistics.median(a), 5), torch_ms=round(statistics.median(b), 5),
                kernels_all_ms=[round(t, 5) for t in a], torch_all_ms=[round(t, 5) for t in b])


def _events(fn, names, dev, n=20):
    """GPU ms per call of the entry points ``names`` (HIP events around each call), median over n runs of fn"""
    from neuralsim_amd import _lib
    fn()
    _sync(dev)
    _lib.TIMER = _lib.KernelTimer(only=names)
    try:
        for _ in range(n):
            fn()
        _sync(dev)
        out = {k: round(statistics.median(a.elapsed_time(b) for a, b in evs), 5) for k, evs in _lib.TIMER.events.items()}
    finally:
        _lib.TIMER = None
    return out


# ------------------------------------------------------------------------------------------------ the reference in torch
def torch_rays(thetas, phis, c2w, mode, axis):
    """lidars.py:211-230"""
    dx, dy, dz = c2w[:3, 0], c2w[:3, 1], c2w[:3, 2]
    Ts, Ps = torch.meshgrid(thetas, phis, indexing="xy") if mode == "grid" else (thetas, phis)
    if axis:
        d = (torch.cos(Ts))[..., None] * dx + (torch.sin(Ts) * torch.sin(Ps))[..., None] * dy + \
            (torch.sin(Ts) * torch.cos(Ps) * -1)[..., None] * dz
    else:
        d = (torch.sin(Ts) * torch.cos(Ps))[..., None] * dx + (torch.sin(Ts) * torch.sin(Ps))[..., None] * dy + \
            (torch.cos(Ts))[..., None] * dz
    o = torch.tile(c2w[:3, 3], [*Ts.shape, 1]).view(-1, 3)
    return o, torch.nn.functional.normalize(d, dim=-1).view(-1, 3)


def torch_returns(acc, depth, o, d, w2l, rgb=None, ids=None, thr=0.95):
    """render.py:331-346; world -> local as a rotation + translation of the points (``world_transform(pts, inv=True)``)"""
    valid = acc > thr
    ranges = depth[valid]
    pts = o[valid] + d[valid] * depth[valid].unsqueeze(-1)
    local = (w2l[:3, :3] * pts.unsqueeze(-2)).sum(-1) + w2l[:3, 3]
    out = dict(ranges=ranges, pts_world=pts, pts_local=local, mask=acc[valid])
    if rgb is not None:
        out["rgb"] = rgb[valid]
    if ids is not None:
        out["ins_seg"] = ids[valid]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", type=int, default=128)
    ap.add_argument("--azimuths", type=int, default=3600)
    ap.add_argument("--pairs", type=int, default=115010)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--box", type=float, nargs=3, default=[100.0, 20.0, 8.0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", type=int, default=0, metavar="K", help="launch each entry point K times at both sizes and "
                    "exit: the pass to run under `rocprofv3 --kernel-trace --stats` for the kernels' own times")
    ap.add_argument("--emulate", action="store_true", help="run the host-compiled kernels of tests/emu on the CPU: a check of this "
                    "file's logic at a small size, the times mean nothing")
    args = ap.parse_args()
    if args.emulate:
        import ctypes
        sys.path.insert(0, str(ROOT / "tests" / "emu"))
        import build_emu
        from neuralsim_amd import _lib
        lib = _lib.bind(ctypes.CDLL(str(build_emu.build())))
        _lib.get_lib, _lib.stream_handle, _lib.require_device = (lambda: lib), (lambda: 0), (lambda t, name="tensor": None)
    from neuralsim_amd import lidar_sim as ls
    dev = torch.device("cpu") if args.emulate else torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator().manual_seed(0)
    rec = dict(device="emulator" if args.emulate else torch.cuda.get_device_name(dev), iters=args.iters, repeat=args.repeat,
               hbm_peak_bytes_per_s=HBM_PEAK)

    # ---- sensors: an irregular beam table over a full turn; a scan pattern of pairs
    elev = torch.sort(torch.rand(args.beams, generator=g, dtype=torch.float64) * 40.0 - 25.0).values
    az = torch.arange(-args.azimuths // 2, args.azimuths // 2, dtype=torch.float64) / (args.azimuths // 2) * math.pi
    grid = ls.LidarSpec.spinning(elev.numpy(), az.numpy(), near=0.3, far=60.0)
    tt = torch.arange(args.pairs, dtype=torch.float64) / args.pairs
    pairs = ls.LidarSpec.paired(math.pi / 2 - (9.25 * torch.sin(200 * math.pi * tt + 1.57) + 3.25) / 180 * math.pi,
                                12.5 * torch.cos(14400 * math.pi * tt) / 180 * math.pi, near=0.3, far=60.0)
    yaw = 0.3
    c2w = torch.tensor([[math.cos(yaw), -math.sin(yaw), 0.0, -30.0], [math.sin(yaw), math.cos(yaw), 0.0, 1.0],
                        [0.0, 0.0, 1.0, -1.5], [0.0, 0.0, 0.0, 1.0]]).to(dev).contiguous()

    if args.kernels_only:
        for spec in (grid, pairs):
            th, ph = spec.thetas.to(dev), spec.phis.to(dev)
            o, d = ls.lidar_raygen(th, ph, c2w, spec.mode, spec.axis)
            N = o.shape[0]
            run = torch.rand((N + 63) // 64, generator=g).repeat_interleave(64)[:N]
            acc = torch.where(run < 0.67, torch.full([N], 0.999), torch.rand(N, generator=g) * 0.9).to(dev)
            depth, rgb = (torch.rand(N, generator=g) * 50 + 1).to(dev), torch.rand(N, 3, generator=g).to(dev)
            ids, w2l = torch.randint(-1, 40, (N,), generator=g).to(dev), ls.invert_pose(c2w)
            for _ in range(args.kernels_only):
                ls.lidar_raygen(th, ph, c2w, spec.mode, spec.axis)
                ls.lidar_returns(acc, depth, o, d, w2l=w2l, rgb=rgb, ids=ids)
        _sync(dev)
        return

    # ---- 1. ray generation
    rec["raygen"] = {}
    for name, spec in (("grid", grid), ("paired", pairs)):
        th, ph = spec.thetas.to(dev), spec.phis.to(dev)
        ours = lambda: ls.lidar_raygen(th, ph, c2w, spec.mode, spec.axis)                     # noqa: E731
        ref = lambda: torch_rays(th, ph, c2w, spec.mode, spec.axis)                            # noqa: E731
        (o1, d1), (o2, d2) = ours(), ref()
        N = o1.shape[0]
        assert torch.equal(o1, o2) and float((d1 - d2).abs().max()) < 1e-6, "ray generation: the kernel and the torch form disagree"
        r = _ab(ours, ref, args.iters, args.repeat, dev)
        r["n_rays"] = N
        r["bytes"] = 24 * N + 4 * (th.numel() + ph.numel()) + 48          # two [N,3] f32 outputs, the angle tables, the pose
        if not args.emulate:
            gpu = _events(ours, ("nsim_lidar_raygen",), dev)["nsim_lidar_raygen"]
            r["kernel_gpu_ms"] = gpu
            r["hbm_fraction"] = round(r["bytes"] / (gpu * 1e-3) / HBM_PEAK, 4)
        rec["raygen"][name] = r

    # ---- 2. returns compaction of a synthetic sweep (about two thirds returns, in runs like walls and sky)
    rec["returns"] = {}
    for name, spec in (("grid", grid), ("paired", pairs)):
        o, d = ls.lidar_raygen(spec.thetas.to(dev), spec.phis.to(dev), c2w, spec.mode, spec.axis)
        N = o.shape[0]
        run = torch.rand((N + 63) // 64, generator=g).repeat_interleave(64)[:N]
        acc = torch.where(run < 0.67, torch.full([N], 0.999), torch.rand(N, generator=g) * 0.9).to(dev)
        depth = (torch.rand(N, generator=g) * 50 + 1).to(dev)
        rgb, ids = torch.rand(N, 3, generator=g).to(dev), torch.randint(-1, 40, (N,), generator=g).to(dev)
        w2l = ls.invert_pose(c2w)
        w2l4 = torch.cat([w2l, torch.tensor([[0.0, 0.0, 0.0, 1.0]], device=dev)]).contiguous()
        ours = lambda: ls.lidar_returns(acc, depth, o, d, w2l=w2l, rgb=rgb, ids=ids)             # noqa: E731
        ref = lambda: torch_returns(acc, depth, o, d, w2l4, rgb, ids)                          # noqa: E731
        a, b = ours(), ref()
        M = a["n_returns"]
        assert M == b["ranges"].shape[0] and torch.equal(a["ranges"], b["ranges"]) and torch.equal(a["pts_world"], b["pts_world"]) \
            and torch.equal(a["ins_seg"], b["ins_seg"]) and torch.equal(a["rgb"], b["rgb"]), "returns: the kernels and torch disagree"
        assert float((a["pts_local"] - b["pts_local"]).abs().max()) < 1e-4
        r = _ab(ours, ref, args.iters, args.repeat, dev)
        r["n_rays"], r["n_returns"] = N, M
        # count reads acc; emit reads acc, depth and, per return, the two ray rows, rgb and the id; it writes 8 + 4 + 4 + 12 + 12
        # + 12 + 8 bytes per return
        r["bytes"] = 4 * N + 8 * N + M * (24 + 12 + 8) + M * 60
        if not args.emulate:
            ev = _events(ours, ("nsim_lidar_returns_count", "nsim_occgrid_scan", "nsim_lidar_returns_emit"), dev)
            r["kernel_gpu_ms"] = ev
            r["hbm_fraction"] = round(r["bytes"] / (sum(ev.values()) * 1e-3) / HBM_PEAK, 4)
        rec["returns"][name] = r

    # ---- 3. one full sweep of the street model
    from occgrid_bench import street_model
    from neuralsim_amd.renderers.single_volume_renderer import SingleVolumeRenderer
    model = street_model(args.box, dev, **(dict(accel_res=(32, 16, 8), num_pts=2 ** 14) if args.emulate else {}))
    model.ray_query_cfg = dict(query_mode="march_occ_multi_upsample",
                               query_param=dict(nablas_has_grad=False, num_coarse=32, num_fine=[8, 8, 16], upsample_inv_s=64.0,
                                                upsample_inv_s_factors=[1, 4, 16], upsample_use_estimate_alpha=True,
                                                march_cfg=dict(step_size=0.1, max_steps=2048)))
    rend = SingleVolumeRenderer(dict(with_rgb=False, with_normal=False, near=0.3, perturb=False, depth_use_normalized_vw=True)).eval()
    lid = ls.Lidar(grid, device=dev)
    l2w = c2w[:3].contiguous()
    w2l4 = torch.cat([ls.invert_pose(c2w), torch.tensor([[0.0, 0.0, 0.0, 1.0]], device=dev)]).contiguous()

    def sweep_kernels():
        return ls.simulate_lidar_sweep(rend, model, lid, l2w, forward_inv_s=64000.0)

    @torch.no_grad()
    def sweep_torch():
        o, d = torch_rays(lid._angles(0)[0], lid._angles(0)[1], c2w, "grid", 0)
        ret = rend.render(model, rays=[o, d], near=lid.near, far=lid.far, rayschunk=65536, with_rgb=False, with_normal=False,
                          with_env=False, bypass_ray_query_cfg={"forward_inv_s": 64000.0})["rendered"]
        return torch_returns(ret["mask_volume"], ret["depth_volume"], o, d, w2l4)

    a, b = sweep_kernels(), sweep_torch()
    r = _ab(sweep_kernels, sweep_torch, 1, max(3, args.repeat), dev)
    r.update(n_rays=int(a["rays_o"].shape[0]), n_returns=a["n_returns"], n_returns_torch=int(b["ranges"].shape[0]), box=args.box)
    rec["street_sweep"] = r
    if not args.emulate:
        rec["peak_memory_gb"] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
