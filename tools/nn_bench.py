#!/usr/bin/env python
"""Time ``neuralsim_amd.pointcloud.nearest_neighbors`` on synthetic LiDAR-like sweeps (the generator of tests/pointcloud_ref.py:
ground plane + two walls, 1/r^2 density, world coordinates far from the origin), N queries against N points.

Per size and method, after ``--warmup`` untimed runs, the median of ``--repeat`` runs of
  * e2e_ms:     HIP events around the whole operator (workspace allocation, every launch, the int64 index copy);
  * kernels:    HIP events around each C entry point (a separate set of runs: the events add host work);
  * leftover:   queries the grid path handed to the exhaustive pass, and their share;
  * grid:       the resolution the device chose, its cell size, the number of occupied cells and their mean occupancy.
``--sweep`` adds the grid path at other target occupancies / ring caps (the constants of neuralsim_amd/pointcloud.py).
``--chamfer`` times ``chamfer_distance`` of one sweep (two searches + roots); ``--render-context`` times a no-grad render of an
800 x 800 view of the bench model and scales it to the sweep's ray count, for the comparison "metric vs rendering".
The exhaustive path runs up to ``--brute-max`` points.  At the sizes both run, the outputs are compared (torch.equal).
One JSON line per configuration; ``--out`` also writes them to a file.
Usage: python tools/nn_bench.py [--sizes 20000 200000 2000000] [--repeat 7] [--sweep] [--chamfer] [--render-context] [--out FILE]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def _event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return r, e0.elapsed_time(e1)


def measure(x, y, method, warmup, repeat, **kw):
    from neuralsim_amd import _lib, pointcloud
    stats = {}
    run = lambda: pointcloud.nearest_neighbors(x, y, method=method, stats=stats, **kw)
    for _ in range(warmup):
        out = run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeat):
        out, t = _event_ms(run)
        ms.append(t)
    rec = dict(method=method, N=int(x.shape[0]), M=int(y.shape[0]), e2e_ms=round(statistics.median(ms), 4),
               e2e_min_ms=round(min(ms), 4), e2e_max_ms=round(max(ms), 4), repeat=repeat, **{k: v for k, v in kw.items()})
    per = {}
    for _ in range(repeat):
        _lib.TIMER = _lib.KernelTimer(only=["nsim_nn_brute", "nsim_nn_grid_count", "nsim_nn_grid_scan", "nsim_nn_grid_fill",
                                            "nsim_nn_grid_query"])
        try:
            run()
            for k, s in _lib.TIMER.summary().items():
                per.setdefault(k, []).append(s["total_ms"])
        finally:
            _lib.TIMER = None
    rec["kernels_ms"] = {k: round(statistics.median(v), 4) for k, v in per.items()}
    if method == "grid":
        hdr = stats["hdr"].cpu()
        left = int(stats["leftover"])
        h = hdr[15:16].view(torch.float32).item()
        rec.update(leftover=left, leftover_share=round(left / max(1, x.shape[0]), 6), grid_res=hdr[8:11].tolist(),
                   grid_cells=int(hdr[11]), cell_size=round(h, 5), occupied_cells=int(hdr[17]),
                   occupancy=round(int(hdr[6]) / max(1, int(hdr[17])), 3))
    return rec, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[20000, 200000, 2000000])
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--brute-max", type=int, default=200000)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--chamfer", action="store_true")
    ap.add_argument("--render-context", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pointcloud_ref as R
    from neuralsim_amd import pointcloud
    dev = torch.device("cuda", 0)
    lines = []

    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("")

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if args.out:                      # line by line: a later configuration that fails does not lose the earlier ones
            with open(args.out, "a") as f:
                f.write(lines[-1] + "\n")

    emit(dict(gpu=torch.cuda.get_device_name(0), target_occ=pointcloud.GRID_TARGET_OCC, max_rings=pointcloud.GRID_MAX_RINGS,
              max_cells=pointcloud.GRID_MAX_CELLS, auto_brute_pairs=pointcloud.AUTO_BRUTE_PAIRS))
    for n in args.sizes:
        x = torch.as_tensor(R.lidar_cloud(n, 21)).to(dev)
        y = torch.as_tensor(R.lidar_cloud(n, 22)).to(dev)
        rec, g = measure(x, y, "grid", args.warmup, args.repeat)
        if n <= args.brute_max:
            brec, b = measure(x, y, "brute", args.warmup, args.repeat)
            same = bool(torch.equal(g[0], b[0]) and torch.equal(g[1], b[1]))
            brec["equals_grid"] = rec["equals_brute"] = same
            brec["pairs_per_s"] = round(n * n / brec["e2e_ms"] * 1e3, 1)
            emit(brec)
        emit(rec)
        if args.sweep and n <= 200000:
            for occ in (1.0, 2.0, 8.0, 16.0):
                srec, s = measure(x, y, "grid", 1, max(3, args.repeat // 2), target_occ=occ)
                srec["equals_default"] = bool(torch.equal(s[0], g[0]) and torch.equal(s[1], g[1]))
                emit(srec)
            for rings in (1, 2, 8):
                srec, s = measure(x, y, "grid", 1, max(3, args.repeat // 2), max_rings=rings)
                srec["equals_default"] = bool(torch.equal(s[0], g[0]) and torch.equal(s[1], g[1]))
                emit(srec)
        if args.chamfer:
            for _ in range(args.warmup):
                pointcloud.chamfer_distance(x, y)
            ms = [_event_ms(lambda: pointcloud.chamfer_distance(x, y))[1] for _ in range(args.repeat)]
            emit(dict(what="chamfer_distance", N=n, M=n, method="auto", path="brute" if n * n <= pointcloud.AUTO_BRUTE_PAIRS else "grid",
                      e2e_ms=round(statistics.median(ms), 4), repeat=args.repeat))
    if args.render_context:
        import bench
        from neuralsim_amd import eval as nev
        tr = bench.build_trainer(dev, 0, 1)
        for it in range(50):
            tr.train_step(it)
        torch.cuda.synchronize()
        ha = tr.appear[0:1].detach() if getattr(tr, "appear", None) is not None else None
        render = lambda: nev.render_image(tr.renderer, tr.model, tr.intr, tr.c2w, tr.WH, 0, rays_h_appear=ha)
        render()
        ms = [_event_ms(render)[1] for _ in range(3)]
        rays = int(tr.WH[0, 0]) * int(tr.WH[0, 1])
        med = statistics.median(ms)
        emit(dict(what="render_context", model="bench model (BASELINE configs[1]), 800 x 800 view, no grad", rays=rays,
                  render_ms=round(med, 3), ms_per_200k_rays=round(med * 200000 / rays, 3)))


if __name__ == "__main__":
    main()
