#!/usr/bin/env python
"""Time the fused LiDAR ground-truth filter (neuralsim_amd/lidar_filter.py: ``nsim_lidar_filter_count`` -> ``nsim_occgrid_scan`` ->
``nsim_lidar_filter_emit``) at the size of a Waymo frame: 5 lidars merged into ~170 k beams, 5 OpenCV cameras (three 1280 x 1920,
two 886 x 1920) with ignore masks, an AABB, 60 boxes -- one frame, and a 200-frame bank in ONE pass.  Each against THE REFERENCE'S
STEPS IN TORCH OPS ON THE SAME DEVICE (``SceneDataLoader._filter_lidar_gts`` on ``MultiCamBundle.project_pts_in_image``, restated in
this file: four masks, four ``nonzero``s, four rounds of gathers over every column, the [C, N] projection, the [B, N, 3] box
tensor; per frame, as the loader runs it), alternated ``--repeat`` times in one process after a warm-up of each; a timed window
is ``--iters`` calls between two device synchronisations under the host clock, medians of the per-call times.  Also recorded: the
bytes the fused pass must move (from the shapes), the GPU time per entry point (HIP events, a pass of its own) and from both
the achieved bandwidth as a fraction of the 8 TB/s HBM peak.  ASSERTED: both sides keep the same points up to the undecidable
ones (at most 1e-4 of them).  The times are recorded, not gated.
Usage: python tools/lidar_filter_bench.py [--beams 34000] [--lidars 5] [--frames 200] [--boxes 60] [--iters 200] [--repeat 5]
                                          [--out profiles/lidar_filter_bench.json] [--emulate]"""
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
HBM_PEAK = 8.0e12
CAM_HW = [(1280, 1920), (1280, 1920), (1280, 1920), (886, 1920), (886, 1920)]
CAM_YAW = [0.0, 45.0, -45.0, 90.0, -90.0]
DIST = [0.04, -0.05, 0.0015, -0.0008, 0.01]


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _window(fn, iters, dev):
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


def _events(fn, names, dev, n=10):
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


def _pose(yaw_deg, pos):
    """OpenCV camera-to-world (+z forward) looking along the yaw in the ground plane, slightly down"""
    a = math.radians(yaw_deg)
    fwd = torch.tensor([math.cos(a), math.sin(a), -0.05], dtype=torch.float64)
    fwd = fwd / fwd.norm()
    right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64))
    right = right / right.norm()
    down = torch.linalg.cross(fwd, right)
    m = torch.eye(4, dtype=torch.float64)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, down, fwd, torch.tensor(pos, dtype=torch.float64)
    return m[:3]


def make_frames(F, L, beams, n_boxes, dev, g, small=False):
    """-> columns of the flat bank (frame-sorted), poses, camera tensors, masks, boxes"""
    hw = [(h // 16, w // 16) for h, w in CAM_HW] if small else CAM_HW
    N = L * beams
    az = torch.rand(F * N, generator=g) * (2 * math.pi)
    el = torch.deg2rad(-20.0 + 25.0 * torch.rand(F * N, generator=g))
    d = torch.stack([torch.cos(el) * torch.cos(az), torch.cos(el) * torch.sin(az), torch.sin(el)], dim=-1)
    rng = torch.rand(F * N, generator=g) * 74.0 + 1.0
    rng[torch.rand(F * N, generator=g) < 0.12] = 0.0                     # no return
    li = torch.arange(L).repeat_interleave(beams).repeat(F)
    fi = torch.arange(F).repeat_interleave(N)
    l2w, c2w = [], []
    for f in range(F):
        ego = [0.4 * f, 0.3 * math.sin(0.05 * f), 0.0]
        for l_ in range(L):
            yaw = 0.02 * f + 0.5 * l_
            m = torch.tensor([[math.cos(yaw), -math.sin(yaw), 0.0, ego[0] + 0.5 * l_], [math.sin(yaw), math.cos(yaw), 0.0, ego[1]],
                              [0.0, 0.0, 1.0, 2.0 - 0.2 * l_]], dtype=torch.float64)
            l2w.append(m)
        for c, yaw in enumerate(CAM_YAW):
            c2w.append(_pose(yaw + 1.1 * f * 0.02 * 57.3, [ego[0] + 1.5, ego[1] + 0.1 * c, 1.6]))
    C = len(hw)
    K = torch.stack([torch.tensor([[1.06 * w, 0.0, w / 2 + 3.0], [0.0, 1.06 * w, h / 2 - 5.0], [0.0, 0.0, 1.0]]) for h, w in hw])
    cams = dict(c2w=torch.stack(c2w).view(F, C, 3, 4).float().to(dev), intr=K.expand(F, C, 3, 3).contiguous().to(dev),
                hw=torch.tensor(hw), dist=torch.tensor(DIST).expand(F, C, 5).contiguous().to(dev))
    Hm, Wm = max(h for h, _ in hw), max(w for _, w in hw)
    ign = torch.zeros(F, C, Hm, Wm, dtype=torch.bool, device=dev)
    ign[:, :, Hm // 2:Hm // 2 + Hm // 6, Wm // 4:Wm // 2] = True            # an ego-vehicle-like patch and a band of sky
    ign[:, :, :Hm // 12] = True
    for c, (h, w) in enumerate(hw):
        ign[:, c, h:] = False
        ign[:, c, :, w:] = False
    rows, off = [], [0]
    for f in range(F):
        ctr = (torch.rand(n_boxes, 3, generator=g, dtype=torch.float64) * 2 - 1) * torch.tensor([60.0, 20.0, 1.0]) + \
            torch.tensor([0.4 * f, 0.0, 0.8])
        yaw = torch.rand(n_boxes, generator=g, dtype=torch.float64) * math.pi
        size = torch.tensor([4.6, 2.0, 1.7]) * (0.8 + 0.6 * torch.rand(n_boxes, 3, generator=g, dtype=torch.float64))
        m = torch.zeros(n_boxes, 3, 4, dtype=torch.float64)
        m[:, 0, 0], m[:, 0, 1], m[:, 1, 0], m[:, 1, 1], m[:, 2, 2] = torch.cos(yaw), -torch.sin(yaw), torch.sin(yaw), torch.cos(yaw), 1.0
        m[:, :, 3] = ctr
        rows.append(torch.cat([m.reshape(n_boxes, 12), size], dim=1))
        off.append(off[-1] + n_boxes)
    data = dict(rays_o=torch.zeros(F * N, 3).to(dev), rays_d=d.to(dev), ranges=rng.to(dev), li=li.to(dev))
    return dict(data=data, fi=fi.to(dev), l2w=torch.stack(l2w).view(F, L, 3, 4).float().to(dev), cams=cams, ign=ign,
                aabb=torch.tensor([[-60.0, -50.0, -3.0], [140.0, 50.0, 25.0]]).to(dev), boxes=torch.cat(rows).float().to(dev),
                box_offsets=torch.tensor(off, dtype=torch.int32).to(dev), off=off, N=N, F=F, L=L, C=C)


# ------------------------------------------------------------------------------------------------ the reference in torch
def torch_project(pts, c2w, K, dist, hw_dev, ign, near_clip=1e-4):
    """MultiCamBundle.project_pts_in_image (cameras.py:397-446) with OpenCV intrinsics: pts [N,3] -> mask [C,N]"""
    R, t = c2w[:, :, :3], c2w[:, :, 3]
    q = pts.unsqueeze(0) - t.unsqueeze(1)
    xyz = (R.transpose(-1, -2).unsqueeze(1) * q.unsqueeze(-2)).sum(-1)
    z = xyz[..., 2]
    zs = torch.where(z.abs() < 1e-9, torch.full_like(z, 1e-9), z)
    x, y = xyz[..., 0] / zs, xyz[..., 1] / zs
    k1, k2, p1, p2, k3 = (dist[:, i:i + 1] for i in range(5))
    r2 = x * x + y * y
    cd = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * cd + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * cd + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    u = K[:, 0, 0:1] * xd + K[:, 0, 1:2] * yd + K[:, 0, 2:3]
    v = K[:, 1, 1:2] * yd + K[:, 1, 2:3]
    H, W = hw_dev[:, 0:1], hw_dev[:, 1:2]
    mask = (z > near_clip) & (u < W) & (u >= 0) & (v < H) & (v >= 0)
    inds = mask.nonzero(as_tuple=True)
    ul, vl = u[inds].long(), v[inds].long()
    mask[inds] = ~ign[inds[0], vl, ul]
    return mask


def torch_filter(data, l2w, c2w, K, dist, hw_dev, ign, aabb, boxes):
    """filter_lidar_gts + _filter_lidar_gts (base_loader.py:696-844) of one merged frame"""
    pts = torch.addcmul(data["rays_o"], data["rays_d"], data["ranges"].unsqueeze(-1))
    m = l2w[data["li"]]
    pts = (m[:, :, :3] * pts.unsqueeze(-2)).sum(-1) + m[:, :, 3]
    inds = (data["ranges"] > 0).nonzero().long()[..., 0]
    pts = pts[inds]
    data = {k: v[inds] for k, v in data.items()}
    inds = torch_project(pts, c2w, K, dist, hw_dev, ign).any(dim=0).nonzero().long()[..., 0]
    pts = pts[inds]
    data = {k: v[inds] for k, v in data.items()}
    inds = ((pts >= aabb[0]) & (pts <= aabb[1])).all(dim=-1).nonzero().long()[..., 0]
    pts = pts[inds]
    data = {k: v[inds] for k, v in data.items()}
    if boxes.shape[0]:
        bm = boxes[:, :12].unflatten(-1, (3, 4))
        q = pts.unsqueeze(0) - bm[:, :, 3].unsqueeze(1)
        pio = (bm[:, :, :3].transpose(-1, -2).unsqueeze(1) * q.unsqueeze(-2)).sum(-1)
        lo, hi = -boxes[:, 12:] / 2.0, boxes[:, 12:] / 2.0
        inds = ((pio >= lo.unsqueeze(1)).all(dim=-1) & (pio <= hi.unsqueeze(1)).all(dim=-1)).any(dim=0).logical_not().nonzero().long()[..., 0]
        data = {k: v[inds] for k, v in data.items()}
    return data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", type=int, default=34000, help="beams per lidar (x --lidars = the merged sweep)")
    ap.add_argument("--lidars", type=int, default=5)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--boxes", type=int, default=60)
    ap.add_argument("--iters", type=int, default=200, help="calls per timed window of one frame (a tenth of it for the bank)")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--emulate", action="store_true", help="run the host-compiled kernels of tests/emu on the CPU: a check of this "
                    "file's logic at a small size (images / 16), the times mean nothing")
    args = ap.parse_args()
    if args.emulate:
        import ctypes
        sys.path.insert(0, str(ROOT / "tests" / "emu"))
        import build_emu
        from neuralsim_amd import _lib
        lib = _lib.bind(ctypes.CDLL(str(build_emu.build())))
        _lib.get_lib, _lib.stream_handle, _lib.require_device = (lambda: lib), (lambda: 0), (lambda t, name="tensor": None)
    elif not torch.cuda.is_available():
        raise SystemExit("lidar_filter_bench: no HIP device (use --emulate for a logic check; it measures nothing)")
    from neuralsim_amd import lidar_filter as lf
    dev = torch.device("cpu") if args.emulate else torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator().manual_seed(0)
    rec = dict(device="emulator" if args.emulate else torch.cuda.get_device_name(dev), iters=args.iters, repeat=args.repeat,
               hbm_peak_bytes_per_s=HBM_PEAK, beams_per_frame=args.beams * args.lidars, cameras=[list(x) for x in CAM_HW],
               boxes_per_frame=args.boxes)
    sc = make_frames(args.frames, args.lidars, args.beams, args.boxes, dev, g, small=args.emulate)
    N, F, C = sc["N"], sc["F"], sc["C"]
    cm = sc["cams"]
    hw_dev = cm["hw"].to(dev)
    names = ["opencv"] * C
    bank_cams = lf.CameraSet(cm["c2w"], cm["intr"], cm["hw"].expand(F, C, 2), names, cm["dist"])

    def frame_args(f):
        sl = slice(f * N, (f + 1) * N)
        return dict(data={k: v[sl] for k, v in sc["data"].items()}, l2w=sc["l2w"][f].contiguous(),
                    cams=lf.CameraSet(cm["c2w"][f].contiguous(), cm["intr"][f].contiguous(), cm["hw"], names, cm["dist"][f].contiguous()),
                    ign=sc["ign"][f], boxes=sc["boxes"][sc["off"][f]:sc["off"][f + 1]])

    def bytes_moved(n, kept, c, b):
        # count reads the rays, ranges and the two indices and writes keep; emit reads keep and, per kept point, its row, and
        # writes the row (o, d, range, li); the tables are read once per block and stay in cache
        return n * (12 + 12 + 4 + 8 + 8 + 1) + n + kept * (28 + 8) + kept * (28 + 8) + (n // 256 + 1) * (c * 96 + b * 60)

    # ---- 1. one frame
    fa = frame_args(F // 2)
    ours = lambda: lf.filter_lidar(fa["data"], fa["l2w"], cams=fa["cams"], ignore_mask=fa["ign"], aabb=sc["aabb"], boxes=fa["boxes"])   # noqa: E731
    ref = lambda: torch_filter(fa["data"], fa["l2w"], cm["c2w"][F // 2], cm["intr"][F // 2], cm["dist"][F // 2], hw_dev, fa["ign"],     # noqa: E731
                               sc["aabb"], fa["boxes"])
    a, b = ours(), ref()
    Mk, Mt = int(a["ranges"].shape[0]), int(b["ranges"].shape[0])
    assert abs(Mk - Mt) <= 1e-4 * N + 1 and Mk > 0, ("one frame: the kernels and torch disagree", Mk, Mt)
    if Mk == Mt:
        assert torch.equal(a["ranges"], b["ranges"]) and torch.equal(a["li"], b["li"]) and torch.equal(a["rays_d"], b["rays_d"])
    r = _ab(ours, ref, args.iters, args.repeat, dev)
    r.update(n_points=N, kept=Mk, kept_torch=Mt, bytes=bytes_moved(N, Mk, C, args.boxes))
    entry = ("nsim_lidar_filter_count", "nsim_occgrid_scan", "nsim_lidar_filter_emit")
    if not args.emulate:
        ev = _events(ours, entry, dev)
        r["kernel_gpu_ms"] = ev
        r["hbm_fraction"] = round(r["bytes"] / (sum(ev.values()) * 1e-3) / HBM_PEAK, 4)
    rec["one_frame"] = r

    # ---- 2. the bank: one fused pass over all frames vs the reference's per-frame loop
    def bank_ours():
        return lf.filter_lidar_bank(sc["data"], sc["l2w"], frame_inds=sc["fi"], cams=bank_cams, ignore_mask=sc["ign"], aabb=sc["aabb"],
                                    boxes=sc["boxes"], box_offsets=sc["box_offsets"])
    per = [frame_args(f) for f in range(F)]

    def bank_ref():
        return [torch_filter(p["data"], p["l2w"], cm["c2w"][f], cm["intr"][f], cm["dist"][f], hw_dev, p["ign"], sc["aabb"], p["boxes"])
                for f, p in enumerate(per)]
    a, b = bank_ours(), bank_ref()
    Mk, Mt = int(a["ranges"].shape[0]), sum(int(x["ranges"].shape[0]) for x in b)
    assert abs(Mk - Mt) <= 1e-4 * N * F + 1 and Mk > 0, ("bank: the kernels and torch disagree", Mk, Mt)
    fo = a["frame_offsets"].tolist()
    assert fo[-1] == Mk and len(fo) == F + 1
    r = _ab(bank_ours, bank_ref, max(1, args.iters // 10), args.repeat, dev)
    r.update(n_frames=F, n_points=N * F, kept=Mk, kept_torch=Mt, bytes=bytes_moved(N * F, Mk, C, args.boxes))
    if not args.emulate:
        ev = _events(bank_ours, entry, dev, n=5)
        r["kernel_gpu_ms"] = ev
        r["hbm_fraction"] = round(r["bytes"] / (sum(ev.values()) * 1e-3) / HBM_PEAK, 4)
        rec["peak_memory_gb"] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)
    rec["bank"] = r
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
