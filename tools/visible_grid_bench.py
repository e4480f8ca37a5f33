#!/usr/bin/env python
"""Time the visible-grid extraction (neuralsim_amd/visible_grid.py) on a street-shaped box at octree depth 9: the street model of
tools/occgrid_bench.py (road, kerbs, parked boxes), cameras driving along it, full views rendered once without gradients; the
volume buffers of all ray chunks are kept and both sides work on the same buffers.  Two measurements, each against THE TOOL'S OWN
ALGORITHM WRITTEN IN TORCH OPS ON THE SAME DEVICE (restated in this file), alternated ``--repeat`` times in one process after a
warm-up of each, host clock around work that ends in a device synchronise, medians:
  * marking:  ``add_samples`` over every chunk + ``reduce_voxels``  vs  per chunk ``nonzero`` -> ``searchsorted`` -> two gathers ->
              ``contains`` -> divide -> ``unique(return_counts)`` (extract_visible_grid.py:221-226, visible_grid.py:88-89,119-121)
              and the merge over chunks (``reduce_voxels``, with summed hits);
  * postprocess("dilation" | "close" | "close2")  vs  the N x 26 neighbour index lists on a bool grid (visible_grid.py:166-245),
              both from the same reduced voxel list, both ending with the ascending index list.
ASSERTED: both sides give the same voxels (and hits).  The times are recorded, not gated: neither side had been measured before
the first run of this file.  Also recorded: samples, kept samples, atomics issued after the in-wave run merge (runs / kept), and
the GPU time per entry point of one marking pass and one ``postprocess("close2")`` (HIP events around each call, a pass of its own).
Usage: python tools/visible_grid_bench.py [--depth 9] [--box 100 20 8] [--views 8] [--wh 480 270] [--repeat 5]
                                          [--out profiles/visible_grid_bench.json]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _timed(fn, dev):
    _sync(dev)
    t0 = time.perf_counter()
    r = fn()
    _sync(dev)
    return r, (time.perf_counter() - t0) * 1e3


def street_cameras(box, n_views, W, H, dev):
    """cameras 1.5 m above the road driving along +x, looking ahead and slightly to alternating sides (OpenCV: +z forward, +y down)"""
    hx, hy, hz = (0.5 * float(b) for b in box)
    c2w = torch.eye(4).repeat(n_views, 1, 1)
    for i in range(n_views):
        yaw = 0.35 * (-1.0) ** i
        fwd = torch.tensor([torch.cos(torch.tensor(yaw)), torch.sin(torch.tensor(yaw)), -0.05])
        fwd = fwd / fwd.norm()
        down = torch.tensor([0.0, 0.0, -1.0])
        right = torch.linalg.cross(down, fwd)
        right = right / right.norm()
        down = torch.linalg.cross(fwd, right)
        eye = torch.tensor([-hx + 4.0 + (2 * hx - 30.0) * i / max(n_views - 1, 1), 0.15 * hy * (-1.0) ** i, -hz + 2.5])
        c2w[i, :3, 0], c2w[i, :3, 1], c2w[i, :3, 2], c2w[i, :3, 3] = right, down, fwd, eye
    f = 0.6 * W
    intr = torch.tensor([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1.0]]).repeat(n_views, 1, 1)
    WH = torch.tensor([[W, H]], dtype=torch.long).repeat(n_views, 1)
    return intr.to(dev), c2w.to(dev), WH.to(dev)


@torch.no_grad()
def render_buffers(model, intr, c2w, WH, rayschunk, far):
    from neuralsim_amd import visible_grid as vg
    from neuralsim_amd.eval import all_pixel_xy
    from neuralsim_amd.graphics.cameras import selected_rays
    bufs = []
    for frame in range(intr.shape[0]):
        W, H = int(WH[frame, 0]), int(WH[frame, 1])
        xy = all_pixel_xy(W, H, intr.device)
        o, d = selected_rays(xy, torch.full([xy.shape[0]], frame, dtype=torch.long, device=intr.device), intr, c2w, WH)
        for i in range(0, o.shape[0], rayschunk):
            oc, dc = o[i:i + rayschunk].contiguous(), d[i:i + rayschunk].contiguous()
            vb = vg.view_buffers(model, oc, dc, near=0.1, far=far, forward_inv_s=64000.)
            if vb is not None:
                keep = {k: vb[k].detach().contiguous() for k in ("rays_inds_hit", "pack_infos_hit", "t", "vw_normalized")}
                bufs.append((oc, dc, dict(keep, type="packed")))
    return bufs


# ------------------------------------------------------------------------------------------------ the tool's algorithm in torch
def torch_mark(grid, bufs, thre=0.1):
    G = grid.G
    strides = grid.grid_size.new_tensor([G * G, G, 1])
    vs, hs = [], []
    for o, d, vb in bufs:
        sel = (vb["vw_normalized"] > thre).nonzero()[:, 0]
        t = vb["t"][sel]
        row = torch.searchsorted(vb["pack_infos_hit"][:, 0].contiguous(), sel, right=True) - 1
        r = vb["rays_inds_hit"][row]
        pts = o[r] + d[r] * t[:, None]
        pts = pts[grid.space.contains(pts).nonzero()[:, 0]]
        c = ((pts - grid.grid_center) / grid.voxel_size).to(torch.long).clamp(max=G - 1)
        v, h = (c * strides).sum(-1).unique(return_counts=True)
        vs.append(v)
        hs.append(h)
    v, inv = torch.cat(vs).unique(return_inverse=True)
    return v, torch.zeros_like(v).index_add_(0, inv, torch.cat(hs))


def _offsets(dev):
    r = torch.arange(-1, 2, device=dev)
    o = torch.cartesian_prod(r, r, r)
    return o[(o != 0).any(-1)]                                                   # (26, 3)


def _coords(v, G):
    return torch.stack([v // (G * G), (v // G) % G, v % G], dim=1)


def _torch_dilate(occ, vox, G, offs):
    n = (_coords(vox, G)[:, None] + offs).flatten(0, 1)
    n = n[((n >= 0) & (n < G)).all(-1).nonzero()[:, 0]]
    occ[n[:, 0], n[:, 1], n[:, 2]] = True


def _torch_erode(occ, vox, G, offs):
    d = occ.clone()
    c = (d > 0).nonzero()
    n = c[:, None] + offs                                                        # (N, 26, 3)
    valid = ((n >= 0) & (n < G)).all(-1)
    n = n.clamp(0, G - 1)
    keep = d[n[..., 0], n[..., 1], n[..., 2]].logical_and(valid).all(dim=1)
    occ[c[:, 0], c[:, 1], c[:, 2]] = keep
    occ.view(-1)[vox] = True


def torch_postprocess(vox, G, op):
    """visible_grid.py:217-232 on a bool grid [G, G, G] that holds ``vox`` (``build_accel``) -> ascending indices"""
    offs = _offsets(vox.device)
    occ = torch.zeros([G, G, G], dtype=torch.bool, device=vox.device)
    occ.view(-1)[vox] = True
    _torch_dilate(occ, vox, G, offs)
    if op == "close2":
        _torch_dilate(occ, occ.view(-1).nonzero()[:, 0], G, offs)
    if op in ("close", "close2"):
        if op == "close2":
            _torch_erode(occ, vox, G, offs)
        _torch_erode(occ, vox, G, offs)
    return occ.view(-1).nonzero()[:, 0]


# ------------------------------------------------------------------------------------------------ main
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=9)
    ap.add_argument("--box", type=float, nargs=3, default=[100.0, 20.0, 8.0])
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--wh", type=int, nargs=2, default=[480, 270])
    ap.add_argument("--rayschunk", type=int, default=65536)
    ap.add_argument("--far", type=float, default=60.0)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
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
    from occgrid_bench import street_model
    from neuralsim_amd.visible_grid import VisibleGrid
    dev = torch.device("cpu") if args.emulate else torch.device("cuda", torch.cuda.current_device())
    model = street_model(args.box, dev, **(dict(accel_res=(32, 16, 8), num_pts=2 ** 14) if args.emulate else {}))
    model.ray_query_cfg = dict(query_mode="march_occ_multi_upsample",
                               query_param=dict(nablas_has_grad=False, num_coarse=32, num_fine=[8, 8, 16], upsample_inv_s=64.0,
                                                upsample_inv_s_factors=[1, 4, 16], upsample_use_estimate_alpha=True,
                                                march_cfg=dict(step_size=0.1, max_steps=2048)))
    intr, c2w, WH = street_cameras(args.box, args.views, args.wh[0], args.wh[1], dev)
    bufs, t_render = _timed(lambda: render_buffers(model, intr, c2w, WH, args.rayschunk, args.far), dev)
    S = sum(int(b[2]["t"].shape[0]) for b in bufs)
    n_sel = sum(int((b[2]["vw_normalized"] > 0.1).sum()) for b in bufs)
    space = model.space

    def ours_mark():
        g = VisibleGrid(space, args.depth)
        for o, d, vb in bufs:
            g.add_samples(o, d, vb, thre=0.1)
        return g.reduce_voxels()

    g0 = VisibleGrid(space, args.depth)
    stats = torch.zeros([2], dtype=torch.long, device=dev)
    for o, d, vb in bufs:
        g0.add_samples(o, d, vb, thre=0.1, stats=stats)
    kept, runs = (int(x) for x in stats.tolist())
    rec = dict(device="emulator" if args.emulate else torch.cuda.get_device_name(dev), octree_depth=args.depth, grid=[g0.G] * 3, box=args.box,
               voxel_size=float(g0.voxel_size[0]), views=args.views, wh=args.wh, rayschunk=args.rayschunk, chunks=len(bufs),
               render_ms=round(t_render, 2), n_samples=S, n_above_threshold=n_sel, n_kept_in_box=kept, n_atomics=runs,
               atomics_per_kept_sample=round(runs / max(kept, 1), 4), repeat=args.repeat)
    del g0
    # marking
    ours, ref = ours_mark(), torch_mark(VisibleGrid(space, args.depth), bufs)          # warm-up + the equality check
    v0, h0 = ours.voxels_in_block[0], ours.voxel_hits_in_block[0]
    assert torch.equal(v0, ref[0]) and torch.equal(h0, ref[1]), "marking: the kernels and the torch form disagree"
    assert int(h0.sum()) == kept
    t_ours, t_ref = [], []
    gt = VisibleGrid(space, args.depth)
    for _ in range(args.repeat):
        t_ours.append(_timed(ours_mark, dev)[1])
        t_ref.append(_timed(lambda: torch_mark(gt, bufs), dev)[1])
    rec["marking"] = dict(n_voxels=int(v0.shape[0]), kernels_ms=round(statistics.median(t_ours), 3),
                          torch_ms=round(statistics.median(t_ref), 3), kernels_all_ms=[round(t, 3) for t in t_ours],
                          torch_all_ms=[round(t, 3) for t in t_ref])
    del ours, ref, gt
    # post-processing
    rec["postprocess"] = {}
    for op in ("dilation", "close", "close2"):
        t_ours, t_ref = [], []
        n_out = None
        for it in range(args.repeat + 1):
            g = VisibleGrid(space, args.depth)
            g.voxels_in_block = {0: v0}
            g.build_accel()
            _, t1 = _timed(lambda: g.postprocess(op), dev)
            want, t2 = _timed(lambda: torch_postprocess(v0, g.G, op), dev)
            if it == 0:                                                           # warm-up + the equality check
                assert torch.equal(g.voxels_in_block[0], want), f"postprocess({op}): the kernels and the torch form disagree"
                n_out = int(want.shape[0])
            else:
                t_ours.append(t1)
                t_ref.append(t2)
            del g, want
        rec["postprocess"][op] = dict(n_voxels_out=n_out, kernels_ms=round(statistics.median(t_ours), 3),
                                      torch_ms=round(statistics.median(t_ref), 3), kernels_all_ms=[round(t, 3) for t in t_ours],
                                      torch_all_ms=[round(t, 3) for t in t_ref])
    if not args.emulate:
        # GPU time per entry point (HIP events around each call, a pass of its own): one marking pass and one postprocess("close2")
        from neuralsim_amd import _lib
        for name, fn in (("marking", ours_mark), ("close2", None)):
            g = VisibleGrid(space, args.depth)
            g.voxels_in_block = {0: v0}
            g.build_accel()
            _sync(dev)
            _lib.TIMER = _lib.KernelTimer()
            try:
                (fn or (lambda: g.postprocess("close2")))()
                summ = _lib.TIMER.summary()
            finally:
                _lib.TIMER = None
            rec.setdefault("gpu_ms_per_entry_point", {})[name] = {k: dict(calls=v["calls"], total_ms=round(v["total_ms"], 4))
                                                                  for k, v in summ.items()}
            del g
        rec["peak_memory_gb"] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
