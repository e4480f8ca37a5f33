"""What pose refinement costs (``ray_query_cfg.query_param.rays_has_grad``): forward + backward of one ``ray_query`` of the close-range
LoTD NeRF model (the sizes of tools/nerf_bench.py) and of the EmerNeRF dynamic model without and with its flow field (the sizes of
tools/dynamic_nerf_bench.py / dynamic_flow_bench.py), fp16, once with rays that carry gradients and once without on the same tree --
the difference is the price of the feature -- and as the torch composition that yields the same ray gradient: the samples
``addcmul(o[ridx], t, d[ridx])`` of leaf rays, the encodings' own forward with ``dydx`` (``nsim_lotd_fwd`` / ``nsim_permuto_fwd``) and its
host-side contraction as the position gradient, the decoders, warps and aggregation as torch ops, autograd.  Also
``nsim_lotd_dx_lm`` alone against ``nsim_lotd_fwd`` with ``dydx`` plus the contraction.  The protocol of tools/dynamic_flow_bench.py:
alternated blocks of 5, 8 blocks each after 5 warm-ups, HIP events around a block, medians with [p10, p90].  Needs the MI355X.

    python tools/pose_grad_bench.py --out profiles/pose_grad_bench.json
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.nerf_bench import sh4, yaml_model_params  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--block", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "pose_grad_bench.json"))
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from neuralsim_amd import _lib
    from neuralsim_amd.fields.dynamic_nerf import EmerNeRFOnlyDynamicModel
    from neuralsim_amd.fields.nerf import LoTDNeRFModel
    from neuralsim_amd.graphics.cameras import look_at_cameras, pinhole_selected_rays
    from neuralsim_amd.grid_encodings.permuto import PermutoEncoding
    assert torch.cuda.is_available(), "pose_grad_bench measures on the device"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    R = args.rays
    key = dict(rays_has_grad=True)
    fns, meta = {}, {}

    # ---- LoTDNeRFModel, tools/nerf_bench.py's scene
    ngp = LoTDNeRFModel(**yaml_model_params(20), seed=42).to(dev)
    with torch.no_grad():
        ngp.encoding.flattened_params.uniform_(-0.5, 0.5, generator=torch.Generator(device=dev).manual_seed(1))
    ctr = torch.stack(torch.meshgrid(*[torch.arange(64, device=dev)] * 3, indexing="ij"), -1).float().reshape(-1, 3)
    ball = ((ctr + 0.5) / 32.0 - 1.0).norm(dim=-1) < 0.6
    ngp.accel.occ_val.copy_(ball.view(64, 64, 64).permute(2, 1, 0).reshape(-1).float() * 100.0)
    ngp.accel.pack_bits()
    gen = torch.Generator(device=dev).manual_seed(2)
    intr, c2w, WH = look_at_cameras(V=3, seed=4242, device=dev)
    o, d = pinhole_selected_rays(torch.rand([R, 2], device=dev, generator=gen), torch.randint(0, 3, [R], device=dev, generator=gen),
                                 intr, c2w, WH)
    ngp_tested = ngp.ray_test(o, d, near=0.01, far=None)
    ngp_qp = dict(ngp.ray_query_cfg["query_param"], **key)

    def query_step(model, tested, qp, params, grad):
        td = dict(tested)
        if grad:
            td["rays_o"] = tested["rays_o"].detach().clone().requires_grad_(True)
            td["rays_d"] = tested["rays_d"].detach().clone().requires_grad_(True)
        for p in params:
            p.grad = None
        vb = model.ray_query(ray_tested=td, config=dict(with_rgb=True, perturb=False, query_param=qp))["volume_buffer"]
        loss = vb["opacity_alpha"].sum() + vb["rgb"].sum()
        if "flow_fwd" in vb:
            loss = loss + (vb["flow_fwd"] ** 2).sum() + (vb["flow_bwd_pred_fwd"] ** 2).sum()
        loss.backward()
        return vb

    class EncX(torch.autograd.Function):
        """features of an encoding's own point-major forward, with a gradient to the table and -- the contraction of ``dydx`` -- to x"""

        @staticmethod
        def forward(ctx, x, table, kind, meta, grid16):
            xd = x.detach().float().contiguous()
            n, nf, nd = xd.shape[0], 32, xd.shape[1]
            if kind == "lotd":
                nf = 2 * int(meta.num_levels)
            out = torch.empty([n, nf], dtype=torch.float32, device=dev)
            dydx = torch.empty([n, nf, nd], dtype=torch.float32, device=dev)
            if kind == "lotd":
                _lib.call("nsim_lotd_fwd", _lib.ptr(xd), _lib.ptr(grid16), meta, n, _lib.ptr(out), _lib.ptr(dydx))
            else:
                _lib.call("nsim_permuto_fwd", meta, _lib.ptr(grid16), _lib.ptr(xd), n, _lib.ptr(out), _lib.ptr(dydx))
            ctx.save_for_backward(xd, dydx)
            ctx.kind, ctx.meta, ctx.n_params = kind, meta, table.shape[0]
            return out

        @staticmethod
        def backward(ctx, g):
            xd, dydx = ctx.saved_tensors
            g = g.float().contiguous()
            dgrid = torch.zeros([ctx.n_params], dtype=torch.float32, device=dev)
            if ctx.kind == "lotd":
                _lib.call("nsim_lotd_bwd", _lib.ptr(xd), _lib.ptr(g), None, ctx.meta, xd.shape[0], _lib.ptr(dgrid))
            else:
                _lib.call("nsim_permuto_bwd", ctx.meta, _lib.ptr(xd), xd.shape[0], _lib.ptr(g), _lib.ptr(dgrid))
            return (g.unsqueeze(-1) * dydx).sum(dim=-2), dgrid, None, None, None

    def leaf_samples(tested, t, ridx):
        o_ = tested["rays_o"].detach().clone().requires_grad_(True)
        d_ = tested["rays_d"].detach().clone().requires_grad_(True)
        return o_, d_, torch.addcmul(o_[ridx], t[:, None], d_[ridx])

    def samples_of(model, tested, qp):
        with torch.no_grad():
            r_ = model.ray_query(ray_tested=tested, config=dict(with_rgb=False, perturb=False, query_param=qp), return_details=True)
        return r_["volume_buffer"]["t"].detach(), r_["details"]["ridx"]
    ngp_params = list(ngp.parameters())
    ngp_t, ngp_ridx = samples_of(ngp, ngp_tested, ngp_qp)

    def ngp_torch():
        for p_ in ngp_params:
            p_.grad = None
        m_, step_ = ngp, ngp._step()
        NF = m_.encoding.cfg.out_features
        o_, d_, x = leaf_samples(ngp_tested, ngp_t, ngp_ridx)
        h = EncX.apply(x, m_.encoding.flattened_params, "lotd", m_.meta.lotd, m_.encoding.shadow())
        lo, hi = m_.accel.aabb[0], m_.accel.aabb[1]
        xn = 2.0 * (x - lo) / (hi - lo) - 1.0
        W1, W2 = m_.den_w[:64 * (NF + 3)].view(64, NF + 3), m_.den_w[64 * (NF + 3):].view(32, 64)
        out = torch.relu(torch.cat([h, xn], -1) @ W1.t() + m_.den_b[:64]) @ W2.t() + m_.den_b[64:]
        alpha = 1.0 - torch.exp(-torch.exp(out[:, 0] - 1.0) * step_)
        K1 = 47
        Q1, Q2, Q3 = m_.rad_w[:64 * K1].view(64, K1), m_.rad_w[64 * K1:64 * K1 + 4096].view(64, 64), m_.rad_w[64 * K1 + 4096:].view(3, 64)
        rr = torch.relu(torch.cat([out[:, 1:], sh4(F.normalize(d_, dim=-1)[ngp_ridx])], -1) @ Q1.t() + m_.rad_b[:64])
        rr = torch.relu(rr @ Q2.t() + m_.rad_b[64:128])
        (alpha.sum() + torch.sigmoid(rr @ Q3.t() + m_.rad_b[128:]).sum()).backward()
    fns["ngp_torch_composition"] = ngp_torch
    meta["ngp"] = dict(samples=int(query_step(ngp, ngp_tested, ngp_qp, ngp_params, False)["t"].shape[0]),
                       rays_hit=int(ngp_tested["num_rays"]), levels=ngp.encoding.cfg.num_levels, log2_hashmap_size=20)
    fns["ngp_rays_grad"] = lambda: query_step(ngp, ngp_tested, ngp_qp, ngp_params, True)
    fns["ngp_no_rays_grad"] = lambda: query_step(ngp, ngp_tested, ngp_qp, ngp_params, False)

    # ---- EmerNeRFOnlyDynamicModel without / with flow, tools/dynamic_flow_bench.py's scene
    pac = dict(type="multi_res", coarsest_res=16.0, finest_res=10000.0, n_levels=16, n_feats=2, log2_hashmap_size=19,
               apply_random_shifts_per_level=True)
    fac = dict(pac, finest_res=2000.0, log2_hashmap_size=18)
    aabb = torch.tensor([[-60.0, -30, -6], [60.0, 30, 6]])
    ts_key = torch.arange(100, dtype=torch.float32) * 0.1
    o2 = torch.tensor([-70.0, 0, 0], device=dev) + (torch.rand(R, 3, device=dev) - 0.5) * torch.tensor([4.0, 40, 8], device=dev)
    d2 = F.normalize((torch.rand(R, 3, device=dev) - 0.5) * torch.tensor([100.0, 50, 10], device=dev) - o2, dim=-1)
    ts, ha = torch.rand(R, device=dev) * 9.9, torch.randn(R, 4, device=dev) * 0.3
    for tag, flow in (("dyn", False), ("dyn_flow", True)):
        kw = dict(use_flow_field=True, use_flow_in_obj=True, flow_encoding_cfg=dict(type="permuto", param=dict(permuto_auto_compute_cfg=fac)),
                  flow_decoder_cfg=dict(type="mlp", D=2, W=64)) if flow else dict(use_flow_field=False)
        m = EmerNeRFOnlyDynamicModel(
            dtype="half", n_geometry_feat=64, time_embedding_cfg=dict(dim=1, learnable=False, weight_init=dict(type="linspace", start=-1, end=1)),
            dynamic_encoding_cfg=dict(type="permuto", param=dict(permuto_auto_compute_cfg=pac)),
            dynamic_decoder_cfg=dict(type="mlp", D=1, W=64, activation="relu"),
            radiance_cfg=dict(use_pos=False, use_nablas=False, use_view_dirs=True, D=2, W=64, dir_embed_cfg=dict(type="spherical", degree=4),
                              n_appear_embedding=4),
            accel_cfg=dict(type="occ_grid_dynamic", vox_size=2.0, occ_thre_consider_mean=True, occ_thre=5.0, ema_decay=0.95,
                           init_cfg=dict(mode="constant", constant_value=50.0), update_from_samples_cfg={}),
            ray_query_cfg=dict(query_mode="march_occ", query_param=dict(march_cfg=dict(step_size=0.5, max_steps=4096))), **kw)
        m.populate(aabb=aabb, ts_keyframes=ts_key, accel_n_jump_frames=2, device=dev)
        with torch.no_grad():
            m.encoding.flattened_params.uniform_(-0.5, 0.5)
            if flow:
                m.flow_encoding.flattened_params.uniform_(-0.5, 0.5)
        tested = m.ray_test(o2, d2, near=0.1, rays_ts=ts, rays_h_appear=ha)
        qp = dict(m.ray_query_cfg["query_param"], **key)
        params = list(m.parameters())
        meta[tag] = dict(samples=int(query_step(m, tested, qp, params, False)["t"].shape[0]), rays_hit=int(tested["num_rays"]),
                         levels=[16, 16] if flow else [16], log2_hashmap_size=[19, 18] if flow else [19])
        def twin(cfg_pac, pmeta):       # PermutoEncoding's own table of the same size and value range, the model's scale / shift
            e_ = PermutoEncoding(4, cfg_pac, device=dev, bound=0.5)
            for l in range(16):
                for i in range(4):
                    e_.cfg.meta.scale[l][i], e_.cfg.meta.shift[l][i] = pmeta.scale[l][i], pmeta.shift[l][i]
            return e_
        enc = twin(pac, m.encoding.cfg.pmeta)
        fenc = twin(fac, m.flow_encoding.cfg.pmeta) if flow else None
        dyn_t, dyn_ridx = samples_of(m, tested, qp)

        def dyn_torch(m=m, tested=tested, params=params, enc=enc, fenc=fenc, t_=dyn_t, ridx_=dyn_ridx, flow=flow):
            for p_ in params + [enc.flattened_params] + ([fenc.flattened_params] if flow else []):
                p_.grad = None
            S_, Fh, K1 = t_.shape[0], 32, 84
            o_, d_, x = leaf_samples(tested, t_, ridx_)
            w = m.time_coord(tested["rays_ts"])[ridx_][:, None]
            x4 = torch.cat([x, w], dim=1)
            dw1, dw2 = m.den_w[:64 * Fh].view(64, Fh), m.den_w[64 * Fh:].view(65, 64)
            rw1, rw2, rw3 = m.rad_w[:64 * K1].view(64, K1), m.rad_w[64 * K1:64 * K1 + 4096].view(64, 64), m.rad_w[64 * K1 + 4096:].view(3, 64)
            feats = lambda e_, pts: EncX.apply(pts, e_.flattened_params, "permuto", e_.cfg.meta, e_.shadow())      # noqa: E731
            extra = 0.0
            if flow:
                fw1, fw2, fw3 = m.flow_w[:64 * Fh].view(64, Fh), m.flow_w[64 * Fh:64 * Fh + 4096].view(64, 64), m.flow_w[64 * Fh + 4096:].view(6, 64)

                def flow_torch(pts):
                    a_ = torch.relu(feats(fenc, pts) @ fw1.t() + m.flow_b[:64])
                    return torch.relu(a_ @ fw2.t() + m.flow_b[64:128]) @ fw3.t() + m.flow_b[128:]
                delta, (lo_, hi_) = float(m.time_delta), m.cfgd["time_range"]
                f6 = flow_torch(x4)
                xp = torch.cat([x + f6[:, :3], (w + delta).clamp(max=hi_)], dim=1)
                xm = torch.cat([x + f6[:, 3:], (w - delta).clamp(min=lo_)], dim=1)
                pred = flow_torch(torch.cat([xp, xm], dim=0))
                a = torch.relu(feats(enc, torch.cat([x4, xp, xm], dim=0)) @ dw1.t() + m.den_b[:64])
                a = 0.5 * a[:S_] + 0.25 * a[S_:2 * S_] + 0.25 * a[2 * S_:]
                extra = (f6[:, :3] ** 2).sum() + (pred[S_:, :3] ** 2).sum()
            else:
                a = torch.relu(feats(enc, x4) @ dw1.t() + m.den_b[:64])
            out = a @ dw2.t() + m.den_b[64:]
            alpha = 1.0 - torch.exp(-F.softplus(out[:, 0]) * 0.5)
            rr = torch.cat([out[:, 1:], sh4(F.normalize(d_, dim=-1)[ridx_]), tested["rays_h_appear"][ridx_]], dim=-1)
            rr = torch.relu(rr @ rw1.t() + m.rad_b[:64])
            rr = torch.relu(rr @ rw2.t() + m.rad_b[64:128])
            (alpha.sum() + torch.sigmoid(rr @ rw3.t() + m.rad_b[128:]).sum() + extra).backward()
        fns[f"{tag}_torch_composition"] = dyn_torch
        fns[f"{tag}_rays_grad"] = (lambda m=m, tested=tested, qp=qp, params=params: query_step(m, tested, qp, params, True))
        fns[f"{tag}_no_rays_grad"] = (lambda m=m, tested=tested, qp=qp, params=params: query_step(m, tested, qp, params, False))

    # ---- nsim_lotd_dx_lm alone against nsim_lotd_fwd's dydx and the host-side contraction, on the NGP model's samples
    with torch.no_grad():
        vb = ngp.ray_query(ray_tested=ngp_tested, config=dict(with_rgb=False, perturb=False), return_details=True)
    t, ridx = vb["volume_buffer"]["t"], vb["details"]["ridx"]
    S, NF = int(t.shape[0]), ngp.encoding.cfg.out_features
    oo, dd = ngp_tested["rays_o"].contiguous(), ngp_tested["rays_d"].contiguous()
    x = torch.addcmul(oo[ridx], t[:, None], dd[ridx]).contiguous()
    g16 = ngp.encoding.shadow()
    dh_pl = torch.randn(16, S, 2, device=dev)
    dh_pm = dh_pl.permute(1, 0, 2).reshape(S, 32)[:, :NF].contiguous()
    dx = torch.empty(S, 3, device=dev)
    out_f, dydx = torch.empty(S, NF, device=dev), torch.empty(S, NF, 3, device=dev)
    lm = ngp.meta.lotd

    def dx_lm():
        _lib.call("nsim_lotd_dx_lm", lm, _lib.ptr(g16), None, _lib.ptr(oo), _lib.ptr(dd), _lib.ptr(t), _lib.ptr(ridx), S, _lib.ptr(dh_pl),
                  0, None, _lib.ptr(dx))

    def dx_dydx():
        _lib.call("nsim_lotd_fwd", _lib.ptr(x), _lib.ptr(g16), lm, S, _lib.ptr(out_f), _lib.ptr(dydx))
        return (dh_pm.unsqueeze(-1) * dydx).sum(dim=-2)
    fns["lotd_dx_lm"], fns["lotd_dx_from_dydx"] = dx_lm, dx_dydx

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
    out = dict(tool="pose_grad_bench", device=torch.cuda.get_device_name(0), torch_version=torch.__version__, rays=R, precision="fp16",
               blocks=args.blocks, block=args.block, models=meta,
               **{k: dict(gpu_events_ms=med(evs[k]), host_ms=med(host[k])) for k in fns})
    for tag in ("ngp", "dyn", "dyn_flow"):
        a, b = out[f"{tag}_rays_grad"], out[f"{tag}_no_rays_grad"]
        out[f"{tag}_price_of_ray_gradients"] = dict(
            gpu_events_ms=round(a["gpu_events_ms"]["p50"] - b["gpu_events_ms"]["p50"], 5),
            gpu_events_ratio=round(a["gpu_events_ms"]["p50"] / b["gpu_events_ms"]["p50"], 3),
            host_ms=round(a["host_ms"]["p50"] - b["host_ms"]["p50"], 5))
        out[f"{tag}_ratio_torch_over_hip"] = round(out[f"{tag}_torch_composition"]["gpu_events_ms"]["p50"] / a["gpu_events_ms"]["p50"], 3)
    out["lotd_dx_samples"] = S
    out["ratio_dydx_over_dx_lm"] = round(out["lotd_dx_from_dydx"]["gpu_events_ms"]["p50"] / out["lotd_dx_lm"]["gpu_events_ms"]["p50"], 3)
    line = json.dumps(out)
    print(line)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
