#!/usr/bin/env python
"""Time the instance / class segmentation of the compose renderer (``render_per_obj_individual``) on the multi-object scenario of
neuralsim_amd/scenarios.py: the street background, 8 posed vehicles of the shared batched model, the distant model and the sky,
one 960 x 640 view of the street rig rendered without gradients in ``--rayschunk`` pieces.  Recorded, medians of ``--repeat``
alternated runs in one process after a warm-up of each, host clock around work that ends in a device synchronise (the z-buffer
part is short: a timed window is ``--inner`` passes over the view, the figure is per pass):
  * ``seg_zbuffer``: ``pack_ops.seg_zbuffer`` (one ``nsim_seg_zbuffer`` call per chunk) over the candidates of every chunk of the view,
    captured from one flag-on pass -- against the "before", THE REFERENCE'S STEPS WRITTEN IN TORCH OPS ON THE SAME DEVICE AND THE
    SAME CANDIDATES (restated in this file from app/renderers/buffer_compose_renderer.py:268-311, 427-450, 549-572: per group
    gather, compare, ``nonzero``, ``.any()``, for a batched group ``unique(return_inverse, return_counts)`` + a scatter-min of the
    depths, the ``depth < z_buffer`` test, ``.any()``, three indexed stores; the scatter-min here keeps the lower position on equal
    depths, which the reference leaves open).  ASSERTED: both give the same buffers;
  * the full view (``eval.render_scene_image``) with and without the flag.
The times are recorded, not gated: nothing here had been measured before the first run of this file.  Also recorded: candidates
per view, rays that carry an instance, the GPU time of the ``nsim_seg_zbuffer`` calls of one pass (HIP events, a pass of its own).
Usage: python tools/segmentation_bench.py [--wh 960 640] [--rayschunk 65536] [--repeat 7] [--inner 20] [--threshold 0.6] [--frame 0]
                                          [--out profiles/segmentation_bench.json]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _timed(fn, dev):
    _sync(dev)
    t0 = time.perf_counter()
    r = fn()
    _sync(dev)
    return r, (time.perf_counter() - t0) * 1e3


# ------------------------------------------------------------------------------------------------ the reference's steps in torch
def torch_zbuffer(sources, N, thr, dev):
    ins_buf = torch.full([N], -1, dtype=torch.long, device=dev)
    cls_buf = torch.full([N], -1, dtype=torch.long, device=dev)
    z = torch.full([N], float("inf"), dtype=torch.float32, device=dev)
    for s in sources:
        ri = s["rays_inds"]
        if ri.numel() == 0:                                   # ``if num_rays > 0`` (a Python int of the ray test)
            continue
        batched = s.get("bidx") is not None
        inds = (s["bidx"], ri) if batched else (ri,)
        mask, depth = s["mask"][inds], s["depth"][inds]
        mm = mask > thr
        idx = mm.nonzero().long()[..., 0]
        if not mm.any():
            continue
        rim, dm = ri[idx], depth[idx]
        im = s["ins"][idx] if batched else s["ins"]
        if batched:
            _, inv, cnt = torch.unique(rim, return_counts=True, return_inverse=True)
            if (cnt > 1).any():
                U = cnt.shape[0]
                dmin = torch.full([U], float("inf"), device=dev).scatter_reduce_(0, inv, dm, "amin")
                pos = torch.arange(dm.shape[0], device=dev)
                first = torch.full([U], dm.shape[0], dtype=torch.long, device=dev).scatter_reduce_(
                    0, inv, torch.where(dm == dmin[inv], pos, dm.shape[0]), "amin")
                rim, dm, im = rim[first], dmin, im[first]
        zn = dm < z[rim]
        if zn.any():
            z[rim[zn]] = dm[zn]
            ins_buf[rim[zn]] = im[zn] if batched else im
            cls_buf[rim[zn]] = s["class_ind"]
    return ins_buf, cls_buf, z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wh", type=int, nargs=2, default=[960, 640])
    ap.add_argument("--rayschunk", type=int, default=65536)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20, help="passes over the view's candidates per timed window of the z-buffer part")
    ap.add_argument("--threshold", type=float, default=0.6)
    ap.add_argument("--frame", type=int, default=0)
    ap.add_argument("--vehicles", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--emulate", action="store_true", help="run the host-compiled kernels of tests/emu on the CPU with the small "
                    "models: a check of this file's logic, the times mean nothing")
    args = ap.parse_args()
    if args.emulate:
        import ctypes
        sys.path.insert(0, str(ROOT / "tests" / "emu"))
        import build_emu
        from neuralsim_amd import _lib
        lib = _lib.bind(ctypes.CDLL(str(build_emu.build())))
        _lib.get_lib, _lib.stream_handle, _lib.require_device = (lambda: lib), (lambda: 0), (lambda t, name="tensor": None)
    from neuralsim_amd import _lib, scenarios as scn
    from neuralsim_amd.eval import render_scene_image
    from neuralsim_amd.graphics import pack_ops as po
    from neuralsim_amd.renderers.buffer_compose_renderer import BufferComposeRenderer, Drawable
    dev = torch.device("cpu") if args.emulate else torch.device("cuda", torch.cuda.current_device())
    small, prec = args.emulate, ("f32" if args.emulate else "fp16")
    W, H = args.wh
    B = args.vehicles
    poses = scn.vehicle_poses(B, device=dev)
    street, dm, sm = scn.street_models(dev, prec, 42, small, scn.street_world())
    street.accel.init(street.query_sdf, generator=torch.Generator(device=dev).manual_seed(42))
    vm = scn.vehicle_model(dev, B, prec, 42, small)
    intr, c2w, WH = scn.street_rig(n_ego=2, H=H, W=W, f=0.625 * W, device=dev)
    drawables = [Drawable("street", "Street", street)] + \
        [Drawable(f"car{b}", "Vehicle", vm, rotation=R, translation=t, scale=s) for b, (R, t, s) in enumerate(poses)]
    rend = BufferComposeRenderer(dict(with_rgb=True, with_normal=True, near=0.1, far=200.0, segmentation_threshold=args.threshold))
    ha = torch.zeros([1, 4], device=dev)
    kw = dict(sky_model=sm, distant_model=dm, rays_h_appear=ha, rayschunk=args.rayschunk)

    def view(flag):
        return render_scene_image(rend, drawables, intr, c2w, WH, args.frame, with_segmentation=flag, **kw)

    # one flag-on pass that keeps the candidates of every chunk
    captured, real = [], po.seg_zbuffer

    def capture(sources, N, threshold=0.6, device=None):
        keep = [{k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in s.items()} for s in sources]
        captured.append((keep, int(N)))
        return real(sources, N, threshold, device=device)
    po.seg_zbuffer = capture
    try:
        img = view(True)
    finally:
        po.seg_zbuffer = real
    thr = float(args.threshold)
    n_cand = sum(int(s["rays_inds"].shape[0]) for srcs, _ in captured for s in srcs)
    ins_img = img["ins_seg_mask_buffer"]
    rec = dict(device="emulator" if args.emulate else torch.cuda.get_device_name(dev), wh=[W, H], rays=W * H, rayschunk=args.rayschunk,
               chunks=len(captured), vehicles=B, frame=args.frame, threshold=thr, sources_per_chunk=len(captured[0][0]),
               candidates=n_cand, rays_with_instance=int((ins_img >= 0).sum()),
               instances_seen=sorted(int(v) for v in ins_img.unique().tolist()), instance_ind_map=img["instance_ind_map"],
               class_ind_map=img["class_ind_map"], repeat=args.repeat)

    def ours_all():
        return [real(srcs, N, thr, device=dev) for srcs, N in captured]

    def torch_all():
        return [torch_zbuffer(srcs, N, thr, dev) for srcs, N in captured]
    a, b = ours_all(), torch_all()                                                    # warm-up + the equality check
    for (ai, ac, az), (bi, bc, bz) in zip(a, b):
        assert torch.equal(ai, bi) and torch.equal(ac, bc) and torch.equal(az, bz), "the kernels and the torch form disagree"
    assert torch.equal(torch.cat([x[0] for x in a]), ins_img.reshape(-1))
    t_ours, t_ref = [], []
    inner = max(1, args.inner)
    for _ in range(args.repeat):
        t_ours.append(_timed(lambda: [ours_all() for _ in range(inner)], dev)[1] / inner)
        t_ref.append(_timed(lambda: [torch_all() for _ in range(inner)], dev)[1] / inner)
    rec["seg_zbuffer"] = dict(kernels_ms=round(statistics.median(t_ours), 4), torch_ms=round(statistics.median(t_ref), 4),
                              kernels_all_ms=[round(t, 4) for t in t_ours], torch_all_ms=[round(t, 4) for t in t_ref],
                              passes_per_window=inner,
                              what="one pass = all chunks of the view; host clock around `passes_per_window` passes + a device "
                                   "synchronise, divided by the passes")
    del a, b
    # the full view with and without the flag
    view(False)
    t_on, t_off = [], []
    for _ in range(args.repeat):
        t_off.append(_timed(lambda: view(False), dev)[1])
        t_on.append(_timed(lambda: view(True), dev)[1])
    rec["full_view"] = dict(flag_off_ms=round(statistics.median(t_off), 3), flag_on_ms=round(statistics.median(t_on), 3),
                            flag_off_all_ms=[round(t, 3) for t in t_off], flag_on_all_ms=[round(t, 3) for t in t_on])
    if not args.emulate:
        _sync(dev)
        _lib.TIMER = _lib.KernelTimer(only=["nsim_seg_zbuffer"])
        try:
            ours_all()
            summ = _lib.TIMER.summary()
        finally:
            _lib.TIMER = None
        rec["gpu_ms_per_entry_point"] = {k: dict(calls=v["calls"], total_ms=round(v["total_ms"], 4)) for k, v in summ.items()}
        rec["peak_memory_gb"] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
