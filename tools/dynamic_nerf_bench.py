"""Forward + backward of one query of the dynamic-only EmerNeRF model at the config's size (16 lattice levels, T = 2^19 of
with_gtbox.240212.yaml:290-300, fp16) on a marched sample set: the fused HIP path (nsim_permuto_gather_pts + nsim_dyn_fwd /
nsim_dyn_bwd + nsim_permuto_scatter_pts) against the same formula as a composition of torch ops on the device over the existing
``PermutoEncoding``.  The two alternate in blocks; medians with [p10, p90].  Needs the MI355X.

    python tools/dynamic_nerf_bench.py --out profiles/dynamic_nerf_bench.json
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def sh4(d):
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    import torch
    return torch.stack([
        torch.full_like(x, 0.28209479177387814), -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x,
        1.0925484305920792 * xy, -1.0925484305920792 * yz, 0.94617469575755997 * z2 - 0.31539156525251999, -1.0925484305920792 * xz,
        0.54627421529603959 * x2 - 0.54627421529603959 * y2, 0.59004358992664352 * y * (-3.0 * x2 + y2), 2.8906114426405538 * xy * z,
        0.45704579946446572 * y * (1.0 - 5.0 * z2), 0.3731763325901154 * z * (5.0 * z2 - 3.0), 0.45704579946446572 * x * (1.0 - 5.0 * z2),
        1.4453057213202769 * z * (x2 - y2), 0.59004358992664352 * x * (-x2 + 3.0 * y2)], dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--block", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--log2-hashmap-size", type=int, default=19)
    ap.add_argument("--out", type=str, default=str(Path(__file__).resolve().parent.parent / "profiles" / "dynamic_nerf_bench.json"))
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from neuralsim_amd.fields.dynamic_nerf import EmerNeRFOnlyDynamicModel, _DynFn
    from neuralsim_amd.grid_encodings.permuto import PermutoEncoding
    assert torch.cuda.is_available(), "dynamic_nerf_bench measures on the device"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    pac = dict(type="multi_res", coarsest_res=16.0, finest_res=10000.0, n_levels=16, n_feats=2,
               log2_hashmap_size=args.log2_hashmap_size, apply_random_shifts_per_level=True)
    step = 0.5
    m = EmerNeRFOnlyDynamicModel(
        dtype="half", n_geometry_feat=64, time_embedding_cfg=dict(dim=1, learnable=False, weight_init=dict(type="linspace", start=-1, end=1)),
        dynamic_encoding_cfg=dict(type="permuto", param=dict(permuto_auto_compute_cfg=pac)),
        dynamic_decoder_cfg=dict(type="mlp", D=1, W=64, activation="relu"),
        radiance_cfg=dict(use_pos=False, use_nablas=False, use_view_dirs=True, D=2, W=64, dir_embed_cfg=dict(type="spherical", degree=4),
                          n_appear_embedding=4),
        accel_cfg=dict(type="occ_grid_dynamic", vox_size=2.0, occ_thre_consider_mean=True, occ_thre=5.0, ema_decay=0.95,
                       init_cfg=dict(mode="constant", constant_value=50.0), update_from_samples_cfg={}),
        ray_query_cfg=dict(query_mode="march_occ", query_param=dict(march_cfg=dict(step_size=step, max_steps=4096))))
    aabb = torch.tensor([[-60.0, -30, -6], [60.0, 30, 6]])
    ts_key = torch.arange(100, dtype=torch.float32) * 0.1
    m.populate(aabb=aabb, ts_keyframes=ts_key, accel_n_jump_frames=2, device=dev)
    with torch.no_grad():
        m.encoding.flattened_params.uniform_(-0.5, 0.5)
    R = args.rays
    o = torch.tensor([-70.0, 0, 0], device=dev) + (torch.rand(R, 3, device=dev) - 0.5) * torch.tensor([4.0, 40, 8], device=dev)
    tgt = (torch.rand(R, 3, device=dev) - 0.5) * torch.tensor([100.0, 50, 10], device=dev)
    d = F.normalize(tgt - o, dim=-1)
    ts = torch.rand(R, device=dev) * 9.9
    ha = torch.randn(R, 4, device=dev) * 0.3
    tested = m.ray_test(o, d, near=0.1, rays_ts=ts, rays_h_appear=ha)
    cfg = dict(with_rgb=True, perturb=False)
    ret = m.ray_query(ray_tested=tested, config=cfg, return_details=True)
    ridx = ret["details"]["ridx"]
    t = ret["volume_buffer"]["t"]
    S = int(t.shape[0])
    dd, hh = tested["rays_d"], tested["rays_h_appear"]
    x4 = m._points(m.time_coord(tested["rays_ts"]), S, rays=(tested["rays_o"], dd, t, ridx))

    # ---- the same formula as torch ops over the existing PermutoEncoding (its own table: the same size and value range)
    enc = PermutoEncoding(4, pac, device=dev, bound=0.5)
    pm, em = m.encoding.cfg.pmeta, enc.cfg.meta
    for l in range(16):
        for i in range(4):
            em.scale[l][i], em.shift[l][i] = pm.scale[l][i], pm.shift[l][i]
    Fh, K1 = 32, 84
    dw1, dw2 = m.den_w[:64 * Fh].view(64, Fh), m.den_w[64 * Fh:].view(65, 64)
    db1, db2 = m.den_b[:64], m.den_b[64:]
    rw1, rw2, rw3 = m.rad_w[:64 * K1].view(64, K1), m.rad_w[64 * K1:64 * K1 + 4096].view(64, 64), m.rad_w[64 * K1 + 4096:].view(3, 64)
    rb1, rb2, rb3 = m.rad_b[:64], m.rad_b[64:128], m.rad_b[128:]
    view = sh4(F.normalize(dd, dim=-1))

    def torch_path():
        h = enc(x4)
        a1 = torch.relu(h @ dw1.t() + db1)
        out = a1 @ dw2.t() + db2
        sigma = F.softplus(out[:, 0])
        alpha = 1.0 - torch.exp(-sigma * step)
        r = torch.cat([out[:, 1:], view[ridx], hh[ridx]], dim=-1)
        r = torch.relu(r @ rw1.t() + rb1)
        r = torch.relu(r @ rw2.t() + rb2)
        return alpha, torch.sigmoid(r @ rw3.t() + rb3)

    def hip_path():
        outs = _DynFn.apply(m, m.encoding.flattened_params, m.den_w, m.den_b, m.rad_w, m.rad_b, hh, x4, dd, ridx, step, True)
        return outs[1], outs[2]
    params = [m.encoding.flattened_params, enc.flattened_params, m.den_w, m.den_b, m.rad_w, m.rad_b]

    def run(path):
        for p in params:
            p.grad = None
        alpha, rgb = path()
        (alpha.sum() + rgb.sum()).backward()

    def timed(path, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(n):
            run(path)
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n, e0.elapsed_time(e1) / n
    paths = dict(hip=hip_path, torch=torch_path)
    for p in paths.values():
        for _ in range(args.warmup):
            run(p)
    host, evs = {k: [] for k in paths}, {k: [] for k in paths}
    for _ in range(args.blocks):
        for k, p in paths.items():
            h_, e_ = timed(p, args.block)
            host[k].append(h_)
            evs[k].append(e_)

    def med(xs):
        xs = sorted(xs)
        q = lambda f: round(xs[min(len(xs) - 1, int(f * len(xs)))], 5)          # noqa: E731
        return dict(p50=q(0.5), p10=q(0.1), p90=q(0.9))
    with torch.no_grad():
        a_h, c_h = hip_path()
    out = dict(tool="dynamic_nerf_bench", device=torch.cuda.get_device_name(0), torch_version=torch.__version__, rays=R, rays_hit=int(tested["num_rays"]),
               samples=S, levels=16, log2_hashmap_size=args.log2_hashmap_size, precision="fp16", blocks=args.blocks, block=args.block,
               alpha_mean=float(a_h.mean()), rgb_mean=float(c_h.mean()),
               **{k: dict(gpu_events_ms=med(evs[k]), host_ms=med(host[k])) for k in paths})
    out["ratio_torch_over_hip"] = dict(gpu_events=round(out["torch"]["gpu_events_ms"]["p50"] / out["hip"]["gpu_events_ms"]["p50"], 3),
                                       host=round(out["torch"]["host_ms"]["p50"] / out["hip"]["host_ms"]["p50"], 3))
    line = json.dumps(out)
    print(line)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
