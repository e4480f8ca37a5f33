"""Forward + backward of one query of the with-flow EmerNeRF model at the config's sizes (fg_emernerf/no_gtbox_with_flow.240208.yaml:
16 + 16 lattice levels, T = 2^19 / 2^18, fp16) on a marched sample set: the fused HIP path (flow gather + nsim_flow_fwd, nsim_dyn_warp,
one dynamic gather over the 3S points + nsim_dyn_fwd_agg, and their backwards with nsim_permuto_dx_pts) against the same formula as a
composition of torch ops on the device over ``PermutoEncoding`` (its position gradient: the host-side contraction of
nsim_permuto_fwd's dydx).  Also ``nsim_permuto_dx_pts`` alone against that contraction.  The protocol of tools/dynamic_nerf_bench.py:
alternated blocks, HIP events, medians with [p10, p90].  Needs the MI355X.

    python tools/dynamic_flow_bench.py --out profiles/dynamic_flow_bench.json
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from tools.dynamic_nerf_bench import sh4  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--block", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=str, default=str(Path(__file__).resolve().parent.parent / "profiles" / "dynamic_flow_bench.json"))
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from neuralsim_amd import _lib
    from neuralsim_amd.fields.dynamic_nerf import EmerNeRFOnlyDynamicModel
    from neuralsim_amd.grid_encodings.permuto import PermutoEncoding
    assert torch.cuda.is_available(), "dynamic_flow_bench measures on the device"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    pac = dict(type="multi_res", coarsest_res=16.0, finest_res=10000.0, n_levels=16, n_feats=2, log2_hashmap_size=19,
               apply_random_shifts_per_level=True)
    fac = dict(pac, finest_res=2000.0, log2_hashmap_size=18)
    step = 0.5
    m = EmerNeRFOnlyDynamicModel(
        dtype="half", n_geometry_feat=64, time_embedding_cfg=dict(dim=1, learnable=False, weight_init=dict(type="linspace", start=-1, end=1)),
        dynamic_encoding_cfg=dict(type="permuto", param=dict(permuto_auto_compute_cfg=pac)),
        dynamic_decoder_cfg=dict(type="mlp", D=1, W=64, activation="relu"),
        use_flow_field=True, use_flow_in_obj=True, flow_encoding_cfg=dict(type="permuto", param=dict(permuto_auto_compute_cfg=fac)),
        flow_decoder_cfg=dict(type="mlp", D=2, W=64),
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
        m.flow_encoding.flattened_params.uniform_(-0.5, 0.5)
    R = args.rays
    o = torch.tensor([-70.0, 0, 0], device=dev) + (torch.rand(R, 3, device=dev) - 0.5) * torch.tensor([4.0, 40, 8], device=dev)
    tgt = (torch.rand(R, 3, device=dev) - 0.5) * torch.tensor([100.0, 50, 10], device=dev)
    d = F.normalize(tgt - o, dim=-1)
    ts = torch.rand(R, device=dev) * 9.9
    ha = torch.randn(R, 4, device=dev) * 0.3
    tested = m.ray_test(o, d, near=0.1, rays_ts=ts, rays_h_appear=ha)
    with torch.no_grad():
        ret = m.ray_query(ray_tested=tested, config=dict(with_rgb=True, perturb=False), return_details=True)
    ridx = ret["details"]["ridx"]
    t = ret["volume_buffer"]["t"]
    S = int(t.shape[0])
    dd, hh = tested["rays_d"], tested["rays_h_appear"]
    x4 = m._points(m.time_coord(tested["rays_ts"]), S, rays=(tested["rays_o"], dd, t, ridx))

    # ---- the same formula as torch ops: PermutoEncoding's own tables (same sizes and value range, the model's scale / shift)
    def twin(cfg_pac, pmeta):
        enc = PermutoEncoding(4, cfg_pac, device=dev, bound=0.5)
        for l in range(16):
            for i in range(4):
                enc.cfg.meta.scale[l][i], enc.cfg.meta.shift[l][i] = pmeta.scale[l][i], pmeta.shift[l][i]
        return enc
    enc, fenc = twin(pac, m.encoding.cfg.pmeta), twin(fac, m.flow_encoding.cfg.pmeta)

    class EncX(torch.autograd.Function):
        """features with a gradient to the table (nsim_permuto_bwd) and to x (dydx of nsim_permuto_fwd, contracted on the host side)"""

        @staticmethod
        def forward(ctx, x, table, e):
            xd = x.detach().float().contiguous()
            n = xd.shape[0]
            out = torch.empty([n, 32], dtype=torch.float32, device=dev)
            dydx = torch.empty([n, 32, 4], dtype=torch.float32, device=dev)
            _lib.call("nsim_permuto_fwd", e.cfg.meta, _lib.ptr(e.shadow()), _lib.ptr(xd), n, _lib.ptr(out), _lib.ptr(dydx))
            ctx.save_for_backward(xd, dydx)
            ctx.e, ctx.n_params = e, table.shape[0]
            return out

        @staticmethod
        def backward(ctx, g):
            xd, dydx = ctx.saved_tensors
            g = g.float().contiguous()
            dgrid = torch.zeros([ctx.n_params], dtype=torch.float32, device=dev)
            _lib.call("nsim_permuto_bwd", ctx.e.cfg.meta, _lib.ptr(xd), xd.shape[0], _lib.ptr(g), _lib.ptr(dgrid))
            return (g.unsqueeze(-1) * dydx).sum(dim=-2), dgrid, None
    Fh, K1 = 32, 84
    dw1, dw2 = m.den_w[:64 * Fh].view(64, Fh), m.den_w[64 * Fh:].view(65, 64)
    db1, db2 = m.den_b[:64], m.den_b[64:]
    rw1, rw2, rw3 = m.rad_w[:64 * K1].view(64, K1), m.rad_w[64 * K1:64 * K1 + 4096].view(64, 64), m.rad_w[64 * K1 + 4096:].view(3, 64)
    rb1, rb2, rb3 = m.rad_b[:64], m.rad_b[64:128], m.rad_b[128:]
    fw1, fw2, fw3 = m.flow_w[:64 * Fh].view(64, Fh), m.flow_w[64 * Fh:64 * Fh + 4096].view(64, 64), m.flow_w[64 * Fh + 4096:].view(6, 64)
    fb1, fb2, fb3 = m.flow_b[:64], m.flow_b[64:128], m.flow_b[128:]
    view = sh4(F.normalize(dd, dim=-1))
    delta, (lo, hi) = float(m.time_delta), m.cfgd["time_range"]

    def flow_torch(x):
        a = torch.relu(EncX.apply(x, fenc.flattened_params, fenc) @ fw1.t() + fb1)
        return torch.relu(a @ fw2.t() + fb2) @ fw3.t() + fb3

    def torch_path():
        f6 = flow_torch(x4)
        w = x4[:, 3:]
        xp = torch.cat([x4[:, :3] + f6[:, :3], (w + delta).clamp(max=hi)], dim=1)
        xm = torch.cat([x4[:, :3] + f6[:, 3:], (w - delta).clamp(min=lo)], dim=1)
        pred = flow_torch(torch.cat([xp, xm], dim=0))
        h = EncX.apply(torch.cat([x4, xp, xm], dim=0), enc.flattened_params, enc)
        a = torch.relu(h @ dw1.t() + db1)
        a = 0.5 * a[:S] + 0.25 * a[S:2 * S] + 0.25 * a[2 * S:]
        out = a @ dw2.t() + db2
        sigma = F.softplus(out[:, 0])
        alpha = 1.0 - torch.exp(-sigma * step)
        r = torch.cat([out[:, 1:], view[ridx], hh[ridx]], dim=-1)
        r = torch.relu(r @ rw1.t() + rb1)
        r = torch.relu(r @ rw2.t() + rb2)
        return alpha, torch.sigmoid(r @ rw3.t() + rb3), f6, pred

    def hip_path():
        sigma, alpha, rgb, flow = m._query(hh, x4, dd, ridx, step, True)
        return alpha, rgb, flow["flow_fwd"], flow["flow_bwd_pred_fwd"]
    params = [m.encoding.flattened_params, m.flow_encoding.flattened_params, enc.flattened_params, fenc.flattened_params, m.den_w,
              m.den_b, m.rad_w, m.rad_b, m.flow_w, m.flow_b]

    def run(path):
        for p in params:
            p.grad = None
        alpha, rgb, fa, fb = path()
        (alpha.sum() + rgb.sum() + (fa ** 2).sum() + (fb ** 2).sum()).backward()

    # ---- nsim_permuto_dx_pts alone against the contraction of nsim_permuto_fwd's dydx
    pm = m.encoding.cfg.pmeta
    g16 = m.encoding.shadow()
    dh_pl = torch.randn(16, S, 2, device=dev)
    dh_pm = dh_pl.permute(1, 0, 2).reshape(S, 32).contiguous()
    dx = torch.empty(S, 4, device=dev)
    out_f = torch.empty(S, 32, device=dev)
    dydx = torch.empty(S, 32, 4, device=dev)

    def dx_hip():
        _lib.call("nsim_permuto_dx_pts", pm, _lib.ptr(g16), _lib.ptr(x4), None, S, _lib.ptr(dh_pl), 0, _lib.ptr(dx))

    def dx_dydx():
        _lib.call("nsim_permuto_fwd", enc.cfg.meta, _lib.ptr(enc.shadow()), _lib.ptr(x4), S, _lib.ptr(out_f), _lib.ptr(dydx))
        return (dh_pm.unsqueeze(-1) * dydx).sum(dim=-2)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n, e0.elapsed_time(e1) / n
    fns = dict(hip=lambda: run(hip_path), torch=lambda: run(torch_path), dx_pts=dx_hip, dx_from_dydx=dx_dydx)
    for f in fns.values():
        for _ in range(args.warmup):
            f()
    host, evs = {k: [] for k in fns}, {k: [] for k in fns}
    for _ in range(args.blocks):
        for k, f in fns.items():
            h_, e_ = timed(f, args.block)
            host[k].append(h_)
            evs[k].append(e_)

    def med(xs):
        xs = sorted(xs)
        q = lambda f: round(xs[min(len(xs) - 1, int(f * len(xs)))], 5)          # noqa: E731
        return dict(p50=q(0.5), p10=q(0.1), p90=q(0.9))
    out = dict(tool="dynamic_flow_bench", device=torch.cuda.get_device_name(0), torch_version=torch.__version__, rays=R,
               rays_hit=int(tested["num_rays"]), samples=S, lattice_points=3 * S, levels=[16, 16], log2_hashmap_size=[19, 18],
               precision="fp16", blocks=args.blocks, block=args.block,
               **{k: dict(gpu_events_ms=med(evs[k]), host_ms=med(host[k])) for k in fns})
    out["ratio_torch_over_hip"] = dict(gpu_events=round(out["torch"]["gpu_events_ms"]["p50"] / out["hip"]["gpu_events_ms"]["p50"], 3),
                                       host=round(out["torch"]["host_ms"]["p50"] / out["hip"]["host_ms"]["p50"], 3))
    out["ratio_dydx_over_dx_pts"] = round(out["dx_from_dydx"]["gpu_events_ms"]["p50"] / out["dx_pts"]["gpu_events_ms"]["p50"], 3)
    line = json.dumps(out)
    print(line)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
