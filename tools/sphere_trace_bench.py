"""One 800x800 view of the bench model (bench.py ``build_trainer``: 16 levels x 2^19 entries, 2x64 SDF decoder, sphere of radius
0.75, occupancy grid initialised from the net) rendered three ways: sphere tracing with the persistent kernel
(``k_sphere_trace``), sphere tracing with the host-loop replay (one ``query_sdf`` launch + one advance step in torch per
iteration), and the volume-rendered view (``eval.render_image``).  Prints one JSON line per repeat.

    python tools/sphere_trace_bench.py [--repeats 5] [--preset object|street]

The parent process starts one child per repeat under its own ``timeout`` (a fresh process: allocator and code caches start
cold every time, which is what the run-to-run spread should include) and stops at the first child that fails."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

# app/visualizer/gui_runner_single_cuboid.py:76-104
PRESETS = dict(object=dict(distance_scale=1.0, min_step=0.002, hit_threshold=1e-4, max_march_iters=500),
               street=dict(distance_scale=30.0, min_step=0.2, hit_threshold=1e-3, max_march_iters=500))


def child(args):
    import torch
    from neuralsim_amd.eval import all_pixel_xy, render_image
    from neuralsim_amd.fields.neus import LoTDNeuSModel
    from neuralsim_amd.fields.sphere_trace import trace_params
    from neuralsim_amd.graphics.cameras import look_at_cameras, pinhole_selected_rays
    from neuralsim_amd.renderers.single_volume_renderer import SingleVolumeRenderer
    dev = torch.device("cuda", 0)
    model = LoTDNeuSModel(sdf_D=2, precision="fp16", ln_inv_s_init=0.5, seed=42).to(dev)
    model.geometric_init_sphere(0.75)
    model.accel.init(model.query_sdf, generator=torch.Generator(device=dev).manual_seed(42))
    intr, c2w, WH = look_at_cameras(V=3, seed=4242, device=dev)
    W, H = int(WH[0, 0]), int(WH[0, 1])
    xy = all_pixel_xy(W, H, dev)
    o, d = pinhole_selected_rays(xy, torch.zeros([xy.shape[0]], dtype=torch.long, device=dev), intr, c2w, WH)
    tested = model.ray_test(o, d, near=0.01, far=None)
    tr = model.tracer
    prm = trace_params(PRESETS[args.preset])
    ro, rd, near, far = tr._rays(tested)

    def timed(fn, n):
        fn()                                    # warm-up: code objects, allocator
        torch.cuda.synchronize()
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return sorted(ts)[len(ts) // 2], out
    ms_k, res = timed(lambda: tr.trace_kernel(ro, rd, near, far, prm), args.inner)
    ms_r, rep = timed(lambda: tr.trace_replay(ro, rd, near, far, prm), max(args.inner // 4, 2))
    cfg = dict(query_mode="sphere_trace", query_param=PRESETS[args.preset], with_rgb=True, with_normal=True, _render=True)
    ms_q, _ = timed(lambda: model.ray_query(ray_tested=tested, config=cfg), args.inner)
    renderer = SingleVolumeRenderer(dict(with_rgb=True, with_normal=False, near=0.01)).eval()
    ms_v, _ = timed(lambda: render_image(renderer, model, intr, c2w, WH, 0), max(args.inner // 4, 2))
    n = res["n_steps"].float()
    same = bool(torch.equal(res["status"], rep["status"]) and torch.equal(res["n_steps"], rep["n_steps"]))
    print(json.dumps(dict(preset=args.preset, rays=int(o.shape[0]), rays_tested=int(tested["num_rays"]),
                          ms_kernel=round(ms_k, 3), ms_host_loop=round(ms_r, 3), ms_ray_query_sphere_trace=round(ms_q, 3),
                          ms_volume_view=round(ms_v, 3), n_steps_mean=round(float(n.mean()), 3), n_steps_max=int(n.max()),
                          sdf_queries=int(n.sum()), hit_share=round(float((res["status"] == 1).float().mean()), 4),
                          alive=int((res["status"] == 0).sum()), kernel_equals_host_loop=same)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20, help="timed calls per measurement (the median is reported)")
    ap.add_argument("--preset", choices=list(PRESETS), default="object")
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds for one repeat")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    for _ in range(args.repeats):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, __file__, "--child", "--preset", args.preset,
               "--inner", str(args.inner)]
        rc = subprocess.call(cmd)
        if rc != 0:         # a failed or hung GPU step: start nothing more on the device
            print(f"repeat failed with exit status {rc}: stopping", file=sys.stderr)
            sys.exit(rc)


if __name__ == "__main__":
    main()
