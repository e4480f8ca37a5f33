#!/usr/bin/env python
"""Time ``neuralsim_amd.mesh.extract_mesh_from_model`` on the headline model (BASELINE configs[1] shapes: 16-level LoTD, 2^19
hash entries, 2 x 64 SDF decoder, fp16), trained for ``--train-steps`` steps of the bench workload so that the surface is
not the initial sphere.  Per lattice size N and colour on / off, the median of ``--repeat`` runs of each phase:
  * query_ms:  lattice points generated on the device + the no-grad SDF query, every plane of the grid once;
  * mc_ms:     the marching-cubes chain (4 launches per slab + the one 12-byte read of the slab's totals);
  * mc_kernel_ms: the GPU time of the nsim_mc_* launches alone (HIP events around each call);
  * color_ms:  model.forward at the vertices (colour runs only);
  * d2h_ms:    verts / faces / normals to the host;
  * ply_ms:    the binary PLY write (tmpfs file).
One JSON line per configuration; ``--out`` also writes them to a file.
Usage: python tools/mesh_bench.py [--N 256 512] [--train-steps 300] [--repeat 3] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _sync():
    torch.cuda.synchronize()


def _timed(fn):
    _sync()
    t0 = time.perf_counter()
    r = fn()
    _sync()
    return r, (time.perf_counter() - t0) * 1e3


def run_once(model, N, include_color, slab=None):
    from neuralsim_amd import _lib, mesh
    fill, h, shape, bmin = mesh.model_lattice_fill(model, N)
    nx, ny, nz = shape
    fill_ms = [0.0]

    def timed_fill(k0, n, out):
        _, ms = _timed(lambda: fill(k0, n, out))
        fill_ms[0] += ms

    _lib.TIMER = _lib.KernelTimer(only=["nsim_mc_count", "nsim_mc_scan", "nsim_mc_emit_verts", "nsim_mc_emit_tris"])
    try:
        with torch.no_grad():
            (v, f, nrm), total_ms = _timed(lambda: mesh.marching_cubes(timed_fill, bmin, h, 0.0, shape=shape, slab=slab,
                                                                       device=model.device))
        ks = _lib.TIMER.summary()
    finally:
        _lib.TIMER = None
    rec = dict(N=N, lattice=[nx, ny, nz], points=nx * ny * nz, verts=int(v.shape[0]), faces=int(f.shape[0]),
               color=include_color, query_ms=fill_ms[0], mc_ms=total_ms - fill_ms[0],
               mc_kernel_ms=sum(k["total_ms"] for k in ks.values()),
               mc_kernels={k: dict(calls=s["calls"], total_ms=round(s["total_ms"], 4)) for k, s in ks.items()})
    if include_color:
        def col():
            with torch.no_grad():
                return torch.cat([model.forward(v[s:s + (1 << 20)], -nrm[s:s + (1 << 20)])["rgb"]
                                  for s in range(0, v.shape[0], 1 << 20)])
        c, rec["color_ms"] = _timed(col)
    host, rec["d2h_ms"] = _timed(lambda: (v.cpu().numpy(), f.cpu().numpy(), nrm.cpu().numpy(),
                                          (c.clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy() if include_color else None))
    d = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(dir=d) as td:
        t0 = time.perf_counter()
        mesh.write_ply(os.path.join(td, "m.ply"), host[0], host[1], host[3])
        rec["ply_ms"] = (time.perf_counter() - t0) * 1e3
        rec["ply_bytes"] = os.path.getsize(os.path.join(td, "m.ply"))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--train-steps", type=int, default=300)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--slab", type=int, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    dev = torch.device("cuda", 0)
    tr = bench.build_trainer(dev, 0, 1)
    t0 = time.perf_counter()
    for it in range(args.train_steps):
        tr.train_step(it)
    _sync()
    train_s = time.perf_counter() - t0
    model = tr.model
    print(json.dumps(dict(train_steps=args.train_steps, train_s=round(train_s, 2), gpu=torch.cuda.get_device_name(0))), flush=True)
    run_once(model, 64, True)                       # warm-up: code objects, allocator
    lines = []
    for N in args.N:
        for color in (False, True):
            recs = [run_once(model, N, color, args.slab) for _ in range(args.repeat)]
            med = dict(recs[-1])
            for k in ("query_ms", "mc_ms", "mc_kernel_ms", "color_ms", "d2h_ms", "ply_ms"):
                if k in med:
                    med[k] = round(statistics.median(r[k] for r in recs), 3)
            med["repeat"] = args.repeat
            med["query_gpts_per_s"] = round(med["points"] / med["query_ms"] * 1e-6, 3)
            med["mc_over_query"] = round(med["mc_ms"] / med["query_ms"], 4)
            lines.append(json.dumps(med))
            print(lines[-1], flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
