#!/usr/bin/env python
"""Time the occupancy export (neuralsim_amd/occgrid.py) on a street-shaped model: a cuboid box, a road surface with kerbs and
box-shaped obstacles written by ``geometric_init_fn``, the default 16-level LoTD pyramid (2^19 hash entries, 2 x 64 SDF decoder,
fp16), an occupancy grid refreshed from the net.  ``s = 2``.  Three paths, alternated ``--repeat`` times in one process after a
warm-up of each, host clock around work that ends in a device synchronise, medians:
  * tool:    the algorithm of code_single/tools/extract_occgrid.py as it runs on this package -- 64^3 blocks, 27 queries per voxel
             through ``model.forward_in_obj``, ``nonzero`` and one host copy per block (restated in this file);
  * lattice: ``extract_occupancy_from_model(prune="none")``, every lattice point once;
  * pruned:  ``prune="accel"``.
Recorded per voxel size: n_voxels, n_lattice, n_queried of each path, the occupied counts and whether the results agree (tool ==
lattice as arrays; pruned a subset of lattice, and whether it is equal).  ASSERTED: the query counts -- the tool asks (s + 1)^3
points per voxel, the lattice prod(res_a s + 1) -- and tool == lattice.  The times are recorded, not gated: none was known before
the first run of this file.  Also recorded: the GPU time of the query and of the nsim_occgrid_* launches of the lattice path
(HIP events around each call, a run of its own).
Usage: python tools/occgrid_bench.py [--occ-res 0.2 0.1] [--box 100 20 8] [--repeat 3] [--out profiles/occgrid_bench.json]"""
import argparse
import itertools
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def street_model(box, dev, accel_res=(256, 64, 32), num_pts=2 ** 21):
    from neuralsim_amd.fields.neus import LoTDNeuSModel
    hx, hy, hz = (0.5 * float(b) for b in box)
    aabb = torch.tensor([[-hx, -hy, -hz], [hx, hy, hz]])
    m = LoTDNeuSModel(aabb=aabb, precision="fp16", accel_cfg=dict(resolution=accel_res, occ_val_fn_cfg=dict(inv_s=16.0),
                                                                     update_from_net_cfg=dict(num_steps=4, num_pts=num_pts))).to(dev)

    def target(x):      # a road 1 m above the box floor with 0.15 m kerbs, parked boxes every 12 m on both sides
        road = x[:, 2] - (-hz + 1.0) - 0.15 * (x[:, 1].abs() > 0.3 * hy).float()
        cx = (x[:, 0] / 12.0).round() * 12.0
        q = torch.stack([(x[:, 0] - cx).abs() - 2.2, (x[:, 1].abs() - 0.55 * hy).abs() - 0.9, (x[:, 2] - (-hz + 1.9)).abs() - 0.8], dim=-1)
        car = torch.linalg.norm(q.clamp_min(0.0), dim=-1) + q.max(dim=-1).values.clamp_max(0.0)
        return torch.minimum(road, car)
    with torch.no_grad():
        m.geometric_init_fn(target)
        m.accel.init(m.query_sdf)
    return m


@torch.no_grad()
def tool_algorithm(model, occ_res, s, side=64):
    """extract_occgrid.py:93-147 on this package (identity world transform, unit scale) -> (int64 [M,3] host array, resolution,
    queries asked)"""
    from neuralsim_amd import occgrid
    import numpy as np
    dev = model.device
    aabb_in_world = occgrid.model_world_aabb(model)
    center, radius = (aabb_in_world[1] + aabb_in_world[0]) / 2.0, (aabb_in_world[1] - aabb_in_world[0]) / 2.0
    resolution = ((aabb_in_world[1] - aabb_in_world[0]) / occ_res).long()
    rl = resolution.tolist()
    sub = [torch.arange(s + 1, device=dev, dtype=torch.float) / s for _ in range(3)]
    sub = torch.stack(torch.meshgrid(sub, indexing="ij"), dim=-1).view(-1, 3)
    out, asked = [], 0
    for (ix, iy, iz) in itertools.product(*[range(0, rl[i], side) for i in range(3)]):
        block = [torch.arange(b0, min(b0 + side, rl[i]), device=dev) for i, b0 in enumerate((ix, iy, iz))]
        full = torch.stack(torch.meshgrid(block, indexing="ij"), dim=-1)
        coords = full.float().unsqueeze(-2) + sub[None, None, None, :, :]
        x = ((coords / resolution) * 2 - 1) * radius + center
        sdf = model.forward_in_obj(x, invalid_sdf=float("inf"))["sdf"]
        asked += sdf.numel()
        n_pos = (sdf > 0).sum(dim=-1)
        has = (n_pos < (s + 1) ** 3) & (n_pos > 0) & sdf.isinf().any(dim=-1).logical_not()
        occ = has.nonzero().long() + torch.tensor([ix, iy, iz], dtype=torch.long, device=dev)
        out.append(occ.short().cpu().numpy())
    return np.concatenate(out, axis=0).astype(np.int64), rl, asked


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--occ-res", type=float, nargs="+", default=[0.2, 0.1])
    ap.add_argument("--box", type=float, nargs=3, default=[100.0, 20.0, 8.0])
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from neuralsim_amd import _lib, occgrid
    assert torch.cuda.is_available(), "occgrid_bench measures on the GPU; there is no other path"
    dev = torch.device("cuda", 0)
    s = 2
    model = street_model(args.box, dev)
    recs = []
    paths = dict(tool=lambda r: tool_algorithm(model, r, s),
                 lattice=lambda r: occgrid.extract_occupancy_from_model(model, occ_res=r, subsample_factor=s),
                 pruned=lambda r: occgrid.extract_occupancy_from_model(model, occ_res=r, subsample_factor=s, prune="accel"))
    for occ_res in args.occ_res:
        for fn in paths.values():            # warm-up of every shape
            fn(occ_res)
        ms = {k: [] for k in paths}
        res = {}
        for _ in range(args.repeat):
            for k, fn in paths.items():
                res[k], t = _timed(lambda: fn(occ_res))
                ms[k].append(t)
        tool_occ, rl, asked = res["tool"]
        lat, pr = res["lattice"], res["pruned"]
        n_vox = rl[0] * rl[1] * rl[2]
        n_lat = (rl[0] * s + 1) * (rl[1] * s + 1) * (rl[2] * s + 1)
        assert asked == (s + 1) ** 3 * n_vox and lat["stats"]["n_lattice"] == n_lat, (asked, lat["stats"])
        assert lat["stats"]["n_queried"] == n_lat - lat["stats"]["n_out_of_box"]
        lat_occ, pr_occ = lat["occ_corners"].cpu().numpy().astype(np.int64), pr["occ_corners"].cpu().numpy().astype(np.int64)
        order = np.lexsort((tool_occ[:, 2], tool_occ[:, 1], tool_occ[:, 0]))
        tool_equals_lattice = bool(np.array_equal(tool_occ[order], lat_occ))
        pruned_set, lat_set = set(map(tuple, pr_occ.tolist())), set(map(tuple, lat_occ.tolist()))
        # per-kernel split of the lattice path, a run of its own
        names = ["nsim_occgrid_points", "nsim_lotd_gather_lm", "nsim_field_sdf", "nsim_occgrid_flags", "nsim_occgrid_count",
                 "nsim_occgrid_scan", "nsim_occgrid_emit", "nsim_rows_gather", "nsim_rows_scatter_add"]
        split = {}
        for k in ("lattice", "pruned"):
            _lib.TIMER = _lib.KernelTimer(only=names)
            try:
                paths[k](occ_res)
                split[k] = {n: dict(calls=v["calls"], total_ms=round(v["total_ms"], 3)) for n, v in _lib.TIMER.summary().items()}
            finally:
                _lib.TIMER = None
        rec = dict(gpu=torch.cuda.get_device_name(0), box=args.box, occ_res=occ_res, s=s, resolution=rl, n_voxels=n_vox,
                   n_lattice=n_lat, queries=dict(tool=asked, lattice=lat["stats"]["n_queried"], pruned=pr["stats"]["n_queried"]),
                   query_ratio_tool_over_lattice=round(asked / n_lat, 4), accel_frac_occupied=round(model.accel.frac_occupied(), 4),
                   occupied=dict(tool=int(len(tool_occ)), lattice=int(len(lat_occ)), pruned=int(len(pr_occ))),
                   agree=dict(tool_equals_lattice=tool_equals_lattice, pruned_subset_of_lattice=pruned_set <= lat_set,
                              pruned_equals_lattice=pruned_set == lat_set),
                   ms={k: round(statistics.median(v), 2) for k, v in ms.items()}, ms_all={k: [round(t, 2) for t in v] for k, v in ms.items()},
                   kernel_ms=split, repeat=args.repeat,
                   note="times recorded, not gated: none was known before this run; host clock around a device synchronise, medians")
        print(json.dumps(rec), flush=True)
        assert tool_equals_lattice and pruned_set <= lat_set, rec["agree"]
        recs.append(rec)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(recs, indent=1) + "\n")


if __name__ == "__main__":
    main()
