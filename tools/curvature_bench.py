#!/usr/bin/env python
"""Time the SDF curvature regulariser on the device.

  * the five ``nsim_curv_*`` entry points and, as the yardstick with the same access pattern, ``nsim_eikonal_loss_fwd``, at 2^16
    and 2^20 points: HIP events around ``--calls`` back-to-back launches, the median of ``--repeat`` such windows, per call; the
    bytes each kernel has to move (computed from the shapes below) over that time.  At 2^16 points a launch moves 1.8-3.4 MB: the
    figure is launch-bound and says so; 2^20 is the bandwidth figure.
  * one ``RenderTrainer`` step of the bench model (bench.py ``build_trainer``): the fused launch chain, the autograd path without
    the term and the autograd path with ``w_curvature`` -- alternated in one process, median of ``--steps`` steps each.
One JSON line per measurement; ``--out`` also writes them to a file.
Usage: python tools/curvature_bench.py [--sizes 65536 1048576] [--calls 200] [--repeat 7] [--steps 40] [--no-trainer] [--out FILE]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

# bytes per point: floats read + floats written
BYTES = dict(nsim_curv_shift=(9 + 3) * 4, nsim_curv_angle_fwd=(6 + 1) * 4, nsim_curv_angle_bwd=(6 + 1 + 6) * 4,
             nsim_curv_loss_fwd=6 * 4, nsim_curv_loss_bwd=(6 + 6) * 4, nsim_eikonal_loss_fwd=3 * 4)


def window_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def kernels(n, calls, repeat, dev):
    from neuralsim_amd import _lib
    g = torch.Generator(device=dev).manual_seed(n)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)          # noqa: E731
    n0, n1, dirs, x, gc = r(n, 3), r(n, 3), r(n, 3), r(n, 3).clamp(-1, 1), r(n)
    lo, hi = torch.full([3], -1.0, device=dev), torch.full([3], 1.0, device=dev)
    x2, curv, d0, d1 = torch.empty(n, 3, device=dev), torch.empty(n, device=dev), torch.empty(n, 3, device=dev), torch.empty(n, 3, device=dev)
    out, gout = torch.zeros([], device=dev), torch.ones([1], device=dev)
    c, p = _lib.call, _lib.ptr
    runs = dict(
        nsim_eikonal_loss_fwd=lambda: c("nsim_eikonal_loss_fwd", p(n0), n, p(out)),
        nsim_curv_shift=lambda: c("nsim_curv_shift", p(n0), p(x), p(dirs), p(lo), p(hi), 1e-4, n, p(x2)),
        nsim_curv_angle_fwd=lambda: c("nsim_curv_angle_fwd", p(n0), p(n1), n, p(curv)),
        nsim_curv_angle_bwd=lambda: c("nsim_curv_angle_bwd", p(n0), p(n1), p(gc), n, p(d0), p(d1)),
        nsim_curv_loss_fwd=lambda: c("nsim_curv_loss_fwd", p(n0), p(n1), n, 0.5, p(out)),
        nsim_curv_loss_bwd=lambda: c("nsim_curv_loss_bwd", p(n0), p(n1), n, 0.5, p(gout), p(d0), p(d1)))
    recs = []
    for name, fn in runs.items():
        window_ms(fn, calls)                                         # warm-up
        ms = [window_ms(fn, calls) for _ in range(repeat)]
        med = statistics.median(ms)
        recs.append(dict(kind="kernel", name=name, n=n, calls=calls, repeat=repeat, us=round(med * 1e3, 3),
                         us_min=round(min(ms) * 1e3, 3), us_max=round(max(ms) * 1e3, 3), bytes=BYTES[name] * n,
                         gbytes_per_s=round(BYTES[name] * n / (med * 1e-3) / 1e9, 1)))
    return recs


def trainer_steps(steps, dev):
    import bench
    variants = dict(fused=dict(fused_step=None, w=0.0), autograd=dict(fused_step=False, w=0.0),
                    autograd_curvature=dict(fused_step=False, w=0.05))
    trs = {}
    for k, v in variants.items():
        tr = bench.build_trainer(dev, 0, 1, fused_step=v["fused_step"])
        tr.w_curvature = v["w"]
        trs[k] = tr
    ms = {k: [] for k in trs}
    it = 0
    for rnd in range(steps + 5):
        for k, tr in trs.items():                                    # alternated: the three see the same machine state
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr.train_step(it)
            e1.record()
            torch.cuda.synchronize()
            if rnd >= 5:
                ms[k].append(e0.elapsed_time(e1))
        it += 1
    return [dict(kind="train_step", variant=k, steps=steps, ms=round(statistics.median(v), 4), ms_min=round(min(v), 4),
                 ms_max=round(max(v), 4), num_uniform=trs[k].num_uniform, num_rays=trs[k].num_rays) for k, v in ms.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2 ** 16, 2 ** 20])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--no-trainer", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("curvature_bench: no HIP device is visible; there is nothing to time without one")
    dev = torch.device("cuda", 0)
    recs = []
    for n in args.sizes:
        recs += kernels(n, args.calls, args.repeat, dev)
    if not args.no_trainer:
        recs += trainer_steps(args.steps, dev)
    lines = [json.dumps(r) for r in recs]
    print("\n".join(lines))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
