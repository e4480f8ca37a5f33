"""Close-range LoTD NeRF (fields/nerf.py) at the size of waymo/ngp_withlidar.230814.yaml: 16 levels with 2^20-entry hash
levels, a 64^3 occupancy grid, step 0.1, fp16 -- a with-grad ``ray_query`` + backward for 4096 pixel rays (with_rgb) and,
separately, 4096 LiDAR rays (with_rgb=False), timed per entry point (HIP events) and as whole steps (host clock around a
synchronised step), medians over ``--repeats`` after ``--warmup`` steps in ONE process.

The fused decoders (``nsim_ngp_fwd`` + ``nsim_ngp_bwd``) are compared with the no-new-kernel alternative, built in this tool
only: the same level-major gather, then the two decoders as torch ops on the gathered planes (autograd backward, handing the
plane gradient to ``nsim_lotd_scatter``).  Prints one JSON line.

    python tools/nerf_bench.py [--rays 4096] [--repeats 20] [--warmup 5] [--out profiles/ngp_bench.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def yaml_model_params(log2_T=20, res=64, step=0.1):
    return dict(
        dtype="half",
        encoding_cfg=dict(input_ch=3, lotd_use_cuboid=False,
                          lotd_auto_compute_cfg=dict(type="ngp", target_num_params=32 * 2 ** 20, min_res=16, n_feats=2,
                                                     log2_hashmap_size=log2_T),
                          param_init_cfg=dict(type="uniform_to_type", bound=1.0e-4)),
        extra_pos_embed_cfg=dict(type="identity"),
        density_decoder_cfg=dict(type="mlp", D=1, W=64, output_activation=dict(type="trunc_exp", offset=-1)),
        n_extra_feat_from_output=31,
        radiance_decoder_cfg=dict(use_pos=False, use_view_dirs=True, use_nablas=False, dir_embed_cfg=dict(type="spherical", degree=4),
                                  D=2, W=64),
        accel_cfg=dict(type="occ_grid", resolution=[res] * 3, occ_thre_consider_mean=True, occ_thre=10.0, ema_decay=0.95,
                       init_cfg=dict(mode="constant", constant_value=50.0), update_from_net_cfg=dict(num_steps=4, num_pts=2 ** 20),
                       update_from_samples_cfg={}, n_steps_between_update=16, n_steps_warmup=256),
        ray_query_cfg=dict(query_mode="march_occ", query_param=dict(march_cfg=dict(step_size=step, max_steps=4096))))


def sh4(d):
    import torch
    x, y, z = d.unbind(-1)
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    return torch.stack([
        torch.full_like(x, 0.28209479177387814), -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x,
        1.0925484305920792 * xy, -1.0925484305920792 * yz, 0.94617469575755997 * z2 - 0.31539156525251999, -1.0925484305920792 * xz,
        0.54627421529603959 * x2 - 0.54627421529603959 * y2, 0.59004358992664352 * y * (-3.0 * x2 + y2), 2.8906114426405538 * xy * z,
        0.45704579946446572 * y * (1.0 - 5.0 * z2), 0.3731763325901154 * z * (5.0 * z2 - 3.0), 0.45704579946446572 * x * (1.0 - 5.0 * z2),
        1.4453057213202769 * z * (x2 - y2), 0.59004358992664352 * x * (-x2 + 3.0 * y2)], dim=-1)


def composed_step(model, o, d, t, ridx, step, with_rgb):
    """gather (HIP) -> torch decoders in fp16 autocast on the planes -> autograd -> scatter (HIP): the no-new-kernel alternative"""
    import torch
    from neuralsim_amd import _lib
    S, F = t.shape[0], model.encoding.cfg.out_features
    grid16, _ = model._shadow()
    h_pl = model._gather(grid16, None, o, d, t, ridx, S, t.device)
    h = h_pl[:F // 2, :S].permute(1, 0, 2).reshape(S, F).detach().requires_grad_(True)
    x = torch.addcmul(o[ridx], t[:, None], d[ridx])
    lo, hi = model.accel.aabb[0], model.accel.aabb[1]
    xn = 2.0 * (x - lo) / (hi - lo) - 1.0
    with torch.autocast("cuda", dtype=torch.float16):
        W1 = model.den_w[:64 * (F + 3)].view(64, F + 3)
        W2 = model.den_w[64 * (F + 3):].view(32, 64)
        a1 = torch.relu(torch.cat([h, xn], -1) @ W1.t() + model.den_b[:64])
        out = (a1 @ W2.t() + model.den_b[64:]).float()
        sigma = torch.exp(out[:, 0] - 1.0)
        alpha = 1.0 - torch.exp(-sigma * step)
        loss = alpha.sum()
        if with_rgb:
            K1 = 47
            Q1, Q2, Q3 = model.rad_w[:64 * K1].view(64, K1), model.rad_w[64 * K1:64 * K1 + 4096].view(64, 64), model.rad_w[64 * K1 + 4096:].view(3, 64)
            v = torch.nn.functional.normalize(d, dim=-1)[ridx]
            r = torch.relu(torch.cat([out[:, 1:], sh4(v)], -1) @ Q1.t() + model.rad_b[:64])
            r = torch.relu(r @ Q2.t() + model.rad_b[64:128])
            loss = loss + torch.sigmoid((r @ Q3.t()).float() + model.rad_b[128:]).sum()
    loss.backward()
    dh_pl = torch.zeros([16, S, 2], dtype=torch.float32, device=t.device)
    dh_pl[:F // 2] = h.grad.view(S, F // 2, 2).permute(1, 0, 2)
    dgrid = torch.zeros_like(model.encoding.flattened_params)
    _lib.call("nsim_lotd_scatter", model.meta.lotd, None, o, d, t, ridx, None, S, dh_pl, dh_pl, None, dgrid, 0, 0)
    return dgrid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--log2-hashmap-size", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    from neuralsim_amd import _lib
    from neuralsim_amd.fields.nerf import LoTDNeRFModel
    from neuralsim_amd.graphics.cameras import look_at_cameras, pinhole_selected_rays
    assert torch.cuda.is_available(), "nerf_bench needs a HIP device"
    dev = torch.device("cuda", 0)
    model = LoTDNeRFModel(**yaml_model_params(args.log2_hashmap_size), seed=42).to(dev)
    with torch.no_grad():      # a table that is not all but zero: densities of order 1, an occupancy of a real scene's order
        model.encoding.flattened_params.uniform_(-0.5, 0.5, generator=torch.Generator(device=dev).manual_seed(1))
    acc = model.accel
    gen = torch.Generator(device=dev).manual_seed(2)
    ctr = torch.stack(torch.meshgrid(*[torch.arange(64, device=dev)] * 3, indexing="ij"), -1).float().reshape(-1, 3)
    ball = ((ctr + 0.5) / 32.0 - 1.0).norm(dim=-1) < 0.6        # storage order is x fastest: permute below
    acc.occ_val.copy_(ball.view(64, 64, 64).permute(2, 1, 0).reshape(-1).float() * 100.0)
    acc.pack_bits()
    intr, c2w, WH = look_at_cameras(V=3, seed=4242, device=dev)
    xy = torch.rand([args.rays, 2], device=dev, generator=gen)
    o, d = pinhole_selected_rays(xy, torch.randint(0, 3, [args.rays], device=dev, generator=gen), intr, c2w, WH)
    tested = model.ray_test(o, d, near=0.01, far=None)
    opt = model.training_setup(dict(lr=1e-2, eps=1e-15, betas=[0.9, 0.99]))
    step = model._step()

    def fused_step(with_rgb):
        ret = model.ray_query(ray_tested=tested, config=dict(with_rgb=with_rgb, perturb=True), return_details=True)
        vb = ret["volume_buffer"]
        loss = vb["opacity_alpha"].sum() + (vb["rgb"].sum() if with_rgb else 0.0)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        return ret

    def med(fn, n, warm):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        return dict(p50=ts[len(ts) // 2], p10=ts[len(ts) // 10], p90=ts[(9 * len(ts)) // 10])
    out = dict(tool="nerf_bench", rays=args.rays, levels=model.encoding.cfg.num_levels, n_params=model.encoding.cfg.n_params,
               log2_hashmap_size=args.log2_hashmap_size, step=step, frac_occupied=acc.frac_occupied(), repeats=args.repeats)
    ret = fused_step(True)
    S = int(ret["volume_buffer"]["t"].shape[0])
    out["samples"] = S
    out["pixel_step_ms"] = med(lambda: fused_step(True), args.repeats, args.warmup)
    out["lidar_step_ms"] = med(lambda: fused_step(False), args.repeats, args.warmup)
    out["pixel_plus_lidar_step_ms"] = med(lambda: (fused_step(True), fused_step(False)), args.repeats, args.warmup)
    # per entry point (HIP events around every C-ABI call of the timed steps)
    _lib.TIMER = _lib.KernelTimer()
    for _ in range(args.repeats):
        fused_step(True)
    summ = _lib.TIMER.summary()
    _lib.TIMER = None
    out["entry_points_pixel_ms"] = {k: round(v["avg_ms"], 4) for k, v in sorted(summ.items())}
    out["fused_decoders_ms"] = round(summ["nsim_ngp_fwd"]["avg_ms"] + summ["nsim_ngp_bwd"]["avg_ms"], 4)
    # the composition on the same samples (fixed sample set: jitter 0 both ways)
    t, ridx = ret["volume_buffer"]["t"].detach(), ret["details"]["ridx"]
    oo, dd = tested["rays_o"].contiguous(), tested["rays_d"].contiguous()
    from neuralsim_amd.fields.nerf import _NgpFn

    def fused_on_samples(with_rgb):
        outs = _NgpFn.apply(model, model.encoding.flattened_params, model.den_w, model.den_b, model.rad_w, model.rad_b, None,
                            None, oo, dd, t, ridx, step, with_rgb)
        opt.zero_grad(set_to_none=True)
        (outs[1].sum() + (outs[2].sum() if with_rgb else 0.0)).backward()

    def composed_on_samples(with_rgb):
        opt.zero_grad(set_to_none=True)
        composed_step(model, oo, dd, t, ridx, step, with_rgb)
    for tag, rgb in (("pixel", True), ("lidar", False)):
        out[f"fused_query_{tag}_ms"] = med(lambda: fused_on_samples(rgb), args.repeats, args.warmup)
        out[f"composed_query_{tag}_ms"] = med(lambda: composed_on_samples(rgb), args.repeats, args.warmup)
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
