"""``PermutoNeRFDistantModel`` at the size of permuto_neus.bmvs.230814.yaml: 8192 rays x 64 shells (S = 524288), a 4-D lattice of
16 levels with T = 2^19, fp16 decoders -- one with-grad ``ray_query`` + backward per step, timed per entry point (HIP events
around every C-ABI call, ``_lib.TIMER``), medians of whole steps on the host clock, ``--repeats`` steps after ``--warmup`` in ONE
process.

Compared with what today's other entry points compose for the same planes and the same table gradient:
  * ``nsim_permuto_fwd`` (point-major features) + a transpose into the level-major planes, against ``nsim_permuto_gather_pts``;
  * a transpose of the dh planes + ``nsim_permuto_bwd`` with the cotangents of invalid shells zeroed, against
    ``nsim_permuto_scatter_pts``;
  * the LoTD distant model (4-D pyramid, 12 levels, T = 2^19) on the same rays.
A measurement aid, not a gate.  Prints one JSON line.

    python tools/permuto_distant_bench.py [--rays 8192] [--repeats 20] [--warmup 5] [--out profiles/permuto_distant_bench.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--shells", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    from neuralsim_amd import _lib
    from neuralsim_amd.fields.nerf_distant import LoTDNeRFDistantModel, PermutoNeRFDistantModel
    from neuralsim_amd.graphics.cameras import look_at_cameras, pinhole_selected_rays
    assert torch.cuda.is_available(), "permuto_distant_bench needs a HIP device"
    dev = torch.device("cuda", 0)
    N, K = args.rays, args.shells
    S = N * K
    pm = PermutoNeRFDistantModel(precision="fp16", max_steps=K, seed=7, permuto_auto_compute_cfg=dict(
        type="multi_res", coarsest_res=10.0, finest_res=2000.0, n_levels=16, n_feats=2, log2_hashmap_size=19)).to(dev)
    lm = LoTDNeRFDistantModel(precision="fp16", max_steps=K, seed=7).to(dev)
    gen = torch.Generator(device=dev).manual_seed(2)
    with torch.no_grad():       # tables that are not all but zero
        for m in (pm, lm):
            m.flattened_params.uniform_(-0.5, 0.5, generator=gen)
    intr, c2w, WH = look_at_cameras(V=3, seed=4242, device=dev)
    xy = torch.rand([N, 2], device=dev, generator=gen)
    o, d = pinhole_selected_rays(xy, torch.randint(0, 3, [N], device=dev, generator=gen), intr, c2w, WH)
    near = torch.full([N], 0.01, device=dev)
    ha = torch.zeros([N, 4], device=dev)
    tested = dict(rays_o=o, rays_d=d, near=near, rays_h_appear=ha)

    def step(m):
        for q in m.parameters():
            q.grad = None
        ret = m.ray_query(ray_tested=tested, config=dict(perturb=True), return_details=True)
        vb = ret["volume_buffer"]
        (vb["opacity_alpha"].sum() + vb["rgb"].sum()).backward()
        return ret

    def med(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        return dict(p50=round(ts[len(ts) // 2], 4), p10=round(ts[len(ts) // 10], 4), p90=round(ts[(9 * len(ts)) // 10], 4))

    def entry_points(fn):
        _lib.TIMER = _lib.KernelTimer()
        for _ in range(args.repeats):
            fn()
        torch.cuda.synchronize()
        summ = _lib.TIMER.summary()
        _lib.TIMER = None
        return {k: round(v["avg_ms"], 4) for k, v in sorted(summ.items())}
    out = dict(tool="permuto_distant_bench", rays=N, shells=K, S=S, levels=pm.cfg.num_levels, hashmap_size=pm.cfg.hashmap_size,
               repeats=args.repeats, warmup=args.warmup, device=torch.cuda.get_device_name(0))
    ret = step(pm)
    out["valid_share"] = round(float(ret["volume_buffer"]["valid"].float().mean()), 4)
    out["permuto_step_ms"] = med(lambda: step(pm))
    out["lotd_step_ms"] = med(lambda: step(lm))
    out["permuto_entry_points_ms"] = entry_points(lambda: step(pm))
    out["lotd_entry_points_ms"] = entry_points(lambda: step(lm))
    # the composition from the point-major entry points, on the same points and cotangents
    u4 = ret["details"]["u4"].detach().contiguous()
    valid = ret["volume_buffer"]["valid"].reshape(-1).contiguous()
    grid16, _ = pm._shadow()
    meta, L = pm.cfg.pmeta, pm.cfg.num_levels
    dh_pl = torch.randn([16, S, 2], device=dev, generator=gen)
    feat = torch.empty([S, 2 * L], dtype=torch.float32, device=dev)
    h_pl = torch.empty([16, S, 2], dtype=torch.float32, device=dev)
    dgrid = torch.zeros(pm.cfg.n_params, dtype=torch.float32, device=dev)

    def new_fwd():
        _lib.call("nsim_permuto_gather_pts", meta, _lib.ptr(grid16), _lib.ptr(u4), S, _lib.ptr(h_pl))

    def composed_fwd():
        _lib.call("nsim_permuto_fwd", meta, _lib.ptr(grid16), _lib.ptr(u4), S, _lib.ptr(feat), None)
        h_pl[:L].copy_(feat.view(S, L, 2).permute(1, 0, 2))

    def new_bwd():
        dgrid.zero_()
        _lib.call("nsim_permuto_scatter_pts", meta, _lib.ptr(u4), _lib.ptr(valid), S, _lib.ptr(dh_pl), _lib.ptr(dgrid))

    def composed_bwd():
        dgrid.zero_()
        g = (dh_pl[:L].permute(1, 0, 2) * valid[:, None, None]).reshape(S, 2 * L).contiguous()
        _lib.call("nsim_permuto_bwd", meta, _lib.ptr(u4), S, _lib.ptr(g), _lib.ptr(dgrid))
    for tag, fn in (("gather_pts", new_fwd), ("composed_fwd_plus_transpose", composed_fwd), ("scatter_pts", new_bwd),
                    ("composed_transpose_plus_bwd", composed_bwd)):
        out[f"{tag}_ms"] = med(fn)
    print(json.dumps(out))
    if args.out:
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
