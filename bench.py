#!/usr/bin/env python
"""bench.py -- training rays/s (forward + backward + optimizer) of the NeuS render step on N MI355X.

Contract: ``python bench.py --gpus N --steps K --warmup W`` (N>1: launched by torch.distributed.run, one rank per
GPU over RCCL).  Prints ONE JSON line on rank 0.  A "step" is one full training iteration of
BASELINE.json configs[1] per GPU: 8192 synthetic rays (posed pinhole cameras 800x800) -> ray test -> occupancy
marching + 3-stage NeuS up-sampling -> fused LoTD(L=16,T=2^19)+2x64 SDF MLP+radiance MLP forward -> compositing ->
rgb-mse + eikonal loss -> backward (incl. second-order normal terms) -> gradient all-reduce -> Adam, with the
occupancy-grid refresh every 16 iterations inside the timed region.  Weak scaling: rays per GPU are fixed.

A plain run sets up, warms up, times the K steps and prints the line (``value``, ``ms_per_step`` = the mean timed step).
``--full`` adds everything else the line can carry: the fp16-vs-oracle rendering check (the run exits non-zero when it
fails), the side measurements (``variants``, ``with_distant_model``), the CPU baseline, the per-kernel table and, N > 1,
the exposed all-reduce.  ``--dump-outputs DIR`` writes, after the timed steps, what one step of the timed path computes
from the state the run started from (``dump_step_outputs``) as DIR/<name>.npy.
"""
import argparse
import json
import math
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402

RAYS_PER_GPU = 8192
SPHERE_RADIUS = 0.75
# Algorithmic work per sample point of the field kernels, L=16, F=2, D=2:
#   gather                16 levels x 8 corners x 2 feats x 2 B (fp16)                          = 512 B read
#   forward (with grad)   gather + the saved h / dh-dx planes (128 + 384 B) + 28 B outputs       = 1052 B
#   scatter               256 f32 atomic adds (1024 B RMW) + dh / g planes (256 B) + gn, x (24 B) = 1304 B
#   SDF-branch backward   72 v_mfma_f32_32x32x16_f16 per 32-point tile                           = 73 728 FLOP
#   radiance backward     44 v_mfma_f32_32x32x16_f16 per 32-point tile                           = 45 056 FLOP
def kernel_model(L: int = 16, L4: int = 12):
    """entry point -> (bound, algorithmic work per sample point); L = levels of the close-range pyramid (16: configs[1];
    19: the street config), L4 = levels of the distant model's 4-D pyramid."""
    g = L * 8 * 2 * 2.0                                         # gather: L levels x 8 corners x 2 feats x 2 B (fp16)
    return {
        "nsim_distant_fwd": ("hbm", L4 * 16 * 4 + 128 + 16.0),     # L4 levels x 16 corners x 4 B + planes + outputs
        "nsim_distant_bwd": ("mfma", 56 * 32768 / 32.0),            # 56 MFMA 32x32x16 per 32-point tile
        "nsim_lotd4_scatter": ("hbm", L4 * 16 * 2 * 4 + 128 + 16.0),
        # no-grad SDF query = level-major gather (table reads + 4 B per level of fp16 feature planes written per point) ...
        "nsim_lotd_gather_lm": ("hbm", g + 4.0 * L),
        # ... + the decoder on the planes (12 v_mfma_f32_32x32x16_f16 per 32-point tile at 2x64); with NSIM_SDF_FUSED=1
        # it is the single fused point-major kernel (gather + decoder)
        "nsim_field_sdf": ("hbm", g) if os.environ.get("NSIM_SDF_FUSED", "0") == "1" else ("mfma", 12 * 32768 / 32.0),
        "nsim_field_fwd": ("hbm", g + 20.0 * L + 28.0),            # gather + the saved h (8 B) / f16 dh-dx (12 B) planes per level + outputs
        "nsim_lotd_scatter": ("hbm", 64.0 * L + 16.0 * L + 24.0),  # 16 f32 atomic adds per level (RMW) + dh / g planes + gn, x
        "nsim_field_bwd_sdf": ("mfma", 73728.0),
        "nsim_field_bwd_rad": ("mfma", 45056.0),
    }


KERNEL_MODEL = kernel_model()
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
MFMA_PEAK_TFLOPS = 2500.0      # dense fp16/bf16 MFMA


def build_trainer(device, rank, world, seed=42, distant=False, sky=False, sdf_D=2, precision="fp16", rays_per_gpu=None,
                  fused_step=None, encoding="lotd", ln_inv_s_init=0.5, marched_only=None):
    """BASELINE configs[1] on one rank.  ``precision``: "fp16" (product default = the reference's ``dtype: half``) or
    "f32" (exact-f32 MFMA validation mode of the same kernels, used by the full-size parity tests)."""
    from neuralsim_amd.fields.neus import LoTDNeuSModel
    from neuralsim_amd.graphics.cameras import look_at_cameras
    from neuralsim_amd.trainer import RenderTrainer
    from neuralsim_amd import distributed as ndist
    if encoding == "permuto":       # PermutoNeuSObj at the same table size (16 levels x 2^19 entries x 2 features; row f4)
        from neuralsim_amd.fields.permuto_neus import PermutoNeuSModel
        model = PermutoNeuSModel(permuto_auto_compute_cfg=dict(type="multi_res", n_levels=16, n_feats=2, log2_hashmap_size=19,
                                                               coarsest_res=16.0, finest_res=2000.0),
                                 sdf_D=sdf_D, precision=precision, ln_inv_s_init=0.5, seed=seed).to(device)
        model.geometric_init_sphere(SPHERE_RADIUS, num_iters=300, num_pts=2 ** 15, lr=2e-3)      # geo_init_method: pretrain
        model.encoding.flattened_params.grad = model.sdf_w.grad = model.sdf_b.grad = None
    else:
        model = LoTDNeuSModel(sdf_D=sdf_D, precision=precision, ln_inv_s_init=ln_inv_s_init, seed=seed).to(device)
        if marched_only is not None:        # the sampling semantics, pinned explicitly (neus.marched_only: query_param wins over the env)
            qp_ = dict(model.ray_query_cfg.get("query_param", {}))
            qp_["upsample_on_marched_only"] = bool(marched_only)
            model.ray_query_cfg = dict(model.ray_query_cfg, query_param=qp_)
        # DTU-scan-like pixel coverage: a sphere of radius 0.75 covers ~40 % of the 800x800 views of the camera rig
        # (radius_init 0.5 of the reference config would cover 16 %); see DESIGN.md sec. 7
        model.geometric_init_sphere(SPHERE_RADIUS)
    model.accel.init(model.query_sdf, generator=torch.Generator(device=device).manual_seed(seed))
    ndist.broadcast_module(model)
    intr, c2w, WH = look_at_cameras(V=100, seed=seed, device=device)
    dm = None
    if distant:      # NeRF++ distant-view model of the reference config (dtu yaml :186-247): 64 shells on EVERY ray
        from neuralsim_amd.fields.nerf_distant import LoTDNeRFDistantModel
        dm = LoTDNeRFDistantModel(aabb=model.accel.aabb.detach().cpu(), precision=precision, seed=seed + 7).to(device)
        ndist.broadcast_module(dm)
    sm = None
    if sky:          # directional sky MLP of the street configs (row a16): one 67 -> 256 -> 256 -> 3 query per ray
        from neuralsim_amd.env import SimpleSky
        sm = SimpleSky(n_appear_embedding=4, precision=precision, seed=seed + 11).to(device)
        ndist.broadcast_module(sm)
    # supervision: the analytic image of the same sphere (colour = 0.5 + 0.5 normal, black background) -- multi-view
    # consistent, so the geometry, the occupancy and the sample statistics stay put over any number of steps (with
    # random target colours the surface grows into a solid block within ~40 iterations and the step gets cheaper);
    # NSIM_BENCH_RANDOM_TARGETS=1 restores the random targets.  lr 1e-3 (reference fglr is 1e-2 with warm-up).
    return RenderTrainer(model, intr, c2w, WH, num_rays=int(rays_per_gpu or RAYS_PER_GPU), lr=1e-3, fused_step=fused_step, w_eikonal=0.1, num_uniform=4096,
                         rank=rank, world_size=world, seed=seed, learn_inv_s=False,   # inv_s is scheduled (mix_linear), held at e^5
                         distant_model=dm, sky_model=sm,
                         target_sphere_radius=None if os.environ.get("NSIM_BENCH_RANDOM_TARGETS") == "1" else SPHERE_RADIUS)


def oracle_of(tr, table="master"):
    """oracle.field.FieldParams + occupancy grid carrying exactly the trainer's current weights (test infrastructure:
    only this file's cpu_baseline / parity legs and tests/ use it).  ``table``: "master" = the optimizer's f32 copy of
    the LoTD table; "stored" = the values of the fp16 table the render kernels read -- the reference's parameter dtype
    (``params fp16``), i.e. THE weights of a render; the f32 master is optimizer state of this repo."""
    from oracle import field as ofield
    m = tr.model
    cfg = m.encoding.cfg
    grid = m.encoding.flattened_params if table == "master" else m._shadow()[0].detach().float()
    p = ofield.params_from_flat(cfg.lod_res, int(math.log2(cfg.hashmap_size)), grid, m.sdf_w, m.sdf_b,
                                m.rad_w, m.rad_b, m.ln_inv_s, sdf_D=m.sdf_D, ln_inv_s_factor=m.ln_inv_s_factor)
    # the occupancy the kernels march against: the packed BITFIELD of the last refresh -- not the value grid thresholded now:
    # between refreshes the sampling passes fold their SDFs into the values (``update_from_samples``, bits untouched), and an
    # oracle marching the values saw voxels the kernels do not yet (one grazing ray of 2048 at 0.06, the "worst ray" of
    # profiles/round6_bench_instrumentation.txt)
    bits = m.accel.occ_bits.detach().cpu().to(torch.int64) & 0xFFFFFFFF
    nvox = int(m.accel.occ_val.shape[0])
    occ = ((bits[:, None] >> torch.arange(32)[None, :]) & 1).reshape(-1)[:nvox].to(torch.bool)
    return p, occ


def _sphere_image_cpu(o, d, radius):
    """analytic image of the synthetic scene (same as nsim_sphere_image): 0.5 + 0.5 n at the first hit, else black."""
    b = (o * d).sum(-1)
    c = (o * o).sum(-1) - radius * radius
    disc = b * b - c
    t = -b - torch.sqrt(disc.clamp_min(0))
    hit = (disc > 0) & (t > 0)
    n = torch.nn.functional.normalize(o + t[:, None] * d, dim=-1)
    return torch.where(hit[:, None], 0.5 + 0.5 * n, torch.zeros_like(o))


def cpu_baseline(tr, iters=5, iters_small=3):
    """The oracle (pure-PyTorch restatement of the reference's algorithm, kind 'port') timed on this box's host cores on
    THE SAME STEP the GPU runs: same weights, occupancy grid and camera rig, the full ray batch, the same query mode
    (``march_occ_multi_upsample_compressed``), the analytic-image targets, the uniform eikonal points, backward, Adam over
    every parameter, and 1/16 of an occupancy refresh (4 x 2^20 SDF queries every 16 iterations on the GPU side).
    ``value`` = median of ``iters`` = 5 timed iterations at the bench's ray count (the median of >= 5; a step
    takes ~10-20 s on the GPU box's host cores: about a minute and a half in all); ``configs0`` = the same step at N = 4096 rays
    (BASELINE configs[0], the reference's own CPU-runnable size), median of 3."""
    from oracle import field as ofield, render as orr
    m = tr.model
    p, occ = oracle_of(tr)
    p.requires_grad_(True)
    aabb = m.accel.aabb.detach().cpu()
    res = list(m.accel.resolution)
    res_t = torch.tensor(res, dtype=torch.long)
    scale = res_t.float() / (aabb[1] - aabb[0])
    occ_val = m.accel.occ_val.detach().cpu().clone()
    intr, c2w, WH = tr.intr.cpu(), tr.c2w.cpu(), tr.WH.cpu()
    mode = m.ray_query_cfg.get("query_mode", "")
    compress = mode.endswith("_compressed")
    from neuralsim_amd.fields.neus import marched_only
    mo = marched_only(m.ray_query_cfg.get("query_param", {}))        # the same sampling mode as the GPU step
    opt = torch.optim.Adam(p.tensors(), lr=1e-3, betas=(0.9, 0.99), eps=1e-15)
    g = torch.Generator().manual_seed(7)
    N_full, M_full = tr.num_rays, tr.num_uniform
    n_refresh = m.accel.num_steps * m.accel.num_pts // m.accel.n_steps_between_update

    def step(n_rays, n_uni, n_ref):
        xy = torch.rand(n_rays, 2, generator=g).clamp(1e-6, 1 - 1e-6)
        fidx = torch.randint(0, intr.shape[0], (n_rays,), generator=g)
        jit, jit_c = torch.rand(n_rays, generator=g), torch.rand(n_rays, 64, generator=g)
        x_uni = aabb[0] + torch.rand(n_uni, 3, generator=g) * (aabb[1] - aabb[0])
        x_ref = aabb[0] + torch.rand(n_ref, 3, generator=g) * (aabb[1] - aabb[0])
        t0 = time.perf_counter()
        with torch.no_grad():        # amortised occupancy refresh
            orr.occ_update(occ_val, x_ref, ofield.forward_sdf(x_ref, p), aabb[0], scale, res_t)
        o, d = orr.pinhole_rays(xy, fidx, intr, c2w, WH)
        gt = _sphere_image_cpu(o, d, SPHERE_RADIUS)
        ha = tr.appear.detach().cpu()[fidx]
        ret = orr.ray_query(p, o, d, ha, occ, aabb[0], aabb[1], res, near=0.01, jitter=jit, jitter_c=jit_c,
                            compress=compress, upsample_on_marched_only=mo)
        loss, _ = orr.render_loss(ret, gt, n_rays, w_eikonal=0.1)
        _, nab_u = ofield.forward_sdf_nablas(x_uni, p)
        loss = loss + 0.1 * ((nab_u.norm(dim=-1) - 1.0) ** 2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return time.perf_counter() - t0

    def median_of(n_rays, n):
        ts = sorted(step(n_rays, M_full, n_refresh) for _ in range(n))
        return ts[len(ts) // 2], ts

    step(512, 256, 16384)           # warms the allocator / thread pool (untimed)
    med, ts = median_of(N_full, iters)
    out = dict(value=N_full / med, unit="rays/s", cores=torch.get_num_threads(), kind="port",
               sample=f"median of {len(ts)} timed iterations of the SAME full step ({N_full} rays, {mode}, analytic-image "
                      f"targets, {M_full} uniform eikonal points, backward, Adam over all {sum(t.numel() for t in p.tensors())} "
                      f"parameters, {n_refresh} occupancy-refresh queries = 1/16 of a refresh, upsample_on_marched_only {mo}); pure-PyTorch oracle, f32, "
                      f"{med:.2f} s per step (all: {', '.join(f'{t:.2f}' for t in ts)})")
    if iters_small > 0 and N_full != 4096:
        med0, ts0 = median_of(4096, iters_small)
        out["configs0"] = dict(value=4096 / med0, unit="rays/s", rays=4096, s_per_step=round(med0, 3), iterations=len(ts0),
                               what="BASELINE configs[0] size (4096 rays/iter, the reference's CPU-runnable case), same step")
    return out


# fp16-MFMA rendering vs the f32 oracle on identical rays / weights (eval mode, no perturbation): asserted.
# tests/test_fullsize_parity.py holds the same comparison (plus f32 mode, samples and gradients) under pytest.
PARITY_RAYS = 2048
# Gates: PSNR, the 99th percentile and the maximum of the per-ray colour error.  Measured (round 3, the sampling pass in
# f32-equivalent arithmetic, so both sides integrate over the same sample set): 77 dB, p99 2.5e-4, p99.9 1.3e-3, max 1.0e-2
# (one grazing ray of 2048: the fp16 field differs from the f32 one by ~4e-5 in sdf, times inv_s ~ 150 inside the sigmoid).
# Round 2 (fp16 sampling pass: different sample sets on 3 % of the rays) needed max <= 0.25.
# gate: PSNR (over all but the worst 0.1 % of the rays) >= 60 dB, p99 <= 2e-3, p99.9 <= 1e-2, at most 0.1 % of the rays beyond max_abs_rgb
PARITY_TOL = dict(min_psnr_db=60.0, p99_abs_rgb=2e-3, p999_abs_rgb=1e-2, max_abs_rgb=2e-2)


def convergence_record(dev, rank=0, world=1, steps=3000, checkpoints=(0, 250, 1000, 3000), n_views=3, sdf_D=2):
    """train the bench workload (fused chain, BASELINE configs[1], the bench's own learning rate and occupancy
    schedule) for ``steps`` iterations from the bench's initialisation and score HELD-OUT 800 x 800 views -- cameras of another
    seed than the 100 training views -- against the analytic target image the model is supervised with, the way the reference's
    eval tool scores a run (code_single/tools/eval.py:241-316: per-frame PSNR / SSIM of ``rgb_volume``, then the mean).
    -> dict(psnr_db=[...], ssim=[...] at the checkpoints, rays_per_s of the training in between)."""
    from neuralsim_amd.eval import all_pixel_xy, psnr, render_image, ssim
    from neuralsim_amd.graphics.cameras import look_at_cameras, pinhole_selected_rays
    tr = build_trainer(dev, rank, world, sdf_D=sdf_D)
    intr, c2w, WH = look_at_cameras(V=n_views, seed=4242, device=dev)
    W_, H_ = int(WH[0, 0]), int(WH[0, 1])
    xy = all_pixel_xy(W_, H_, dev)
    gts = []
    for f in range(n_views):
        o_, d_ = pinhole_selected_rays(xy, torch.full([xy.shape[0]], f, dtype=torch.long, device=dev), intr, c2w, WH)
        gts.append(tr.sphere_image(o_, d_, SPHERE_RADIUS).view(H_, W_, 3))
    ha = torch.zeros(1, tr.appear.shape[1], device=dev)          # a held-out view has no appearance code of its own

    def score():
        ps, ss = [], []
        for f in range(n_views):
            img = render_image(tr.renderer, tr.model, intr, c2w, WH, frame=f, rays_h_appear=ha)["rgb_volume"]
            ps.append(psnr(img, gts[f]))
            ss.append(ssim(img, gts[f]))
        return round(sum(ps) / n_views, 2), round(sum(ss) / n_views, 4)
    rec = dict(steps=[], psnr_db=[], ssim=[], train_ms_per_step=[], views=n_views, image="800x800", held_out=True,
               target="analytic image of the supervised sphere (colour = 0.5 + 0.5 normal, black background)")
    it, done = 0, 0
    for cp in checkpoints:
        if cp > done:
            ms, it = time_steps(tr, cp - done, 0, it)
            rec["train_ms_per_step"].append(round(ms, 3))
            done = cp
        p_, s_ = score()
        rec["steps"].append(cp)
        rec["psnr_db"].append(p_)
        rec["ssim"].append(s_)
    rec["rays"] = tr.num_rays
    return rec


def parity_check(tr):
    from oracle import render as orr
    m = tr.model
    p, occ = oracle_of(tr, table="stored")
    aabb = m.accel.aabb.detach().cpu()
    intr, c2w, WH = tr.intr.cpu(), tr.c2w.cpu(), tr.WH.cpu()
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        dev = m.device
        n_par = PARITY_RAYS
        xy = torch.rand(n_par, 2, generator=g).clamp(1e-6, 1 - 1e-6)
        fidx = torch.randint(0, intr.shape[0], (n_par,), generator=g)
        o, d = orr.pinhole_rays(xy, fidx, intr, c2w, WH)
        ha = tr.appear.detach().cpu()[fidx]
        mode = m.ray_query_cfg.get("query_mode", "")
        from neuralsim_amd.fields.neus import marched_only
        ret = orr.ray_query(p, o, d, ha, occ, aabb[0], aabb[1], m.accel.resolution, near=0.01,
                            depth_use_normalized_vw=True, compress=mode.endswith("_compressed"),
                            upsample_on_marched_only=marched_only(m.ray_query_cfg.get("query_param", {})))
        rgb_o = torch.zeros(n_par, 3).index_put((ret["rays_inds"],), ret["rendered"]["rgb_volume"])
        from neuralsim_amd.renderers.single_volume_renderer import SingleVolumeRenderer
        rend = SingleVolumeRenderer(dict(with_rgb=True, near=0.01, depth_use_normalized_vw=True)).eval()
        out = rend.render(m, rays=[o.to(dev), d.to(dev)], rays_h_appear=ha.to(dev))
        rgb_h = out["rendered"]["rgb_volume"].cpu()
        mse = float(((rgb_h - rgb_o) ** 2).mean())
        err = (rgb_h - rgb_o).abs().max(dim=-1).values
        # the gate is on robust statistics -- PSNR over all but the worst 0.1 % of the rays, the 99th and 99.9th percentiles --; the
        # maximum is REPORTED with the number of rays beyond it (a gate on the maximum over 2048 rays made the whole bench exit
        # non-zero when ONE ray differed -- then because the oracle marched another occupancy than the kernels, oracle_of)
        k_trim = max(1, int(0.001 * n_par))
        keep = err.argsort()[:n_par - k_trim]
        mse_trim = float(((rgb_h - rgb_o)[keep] ** 2).mean())
        iw = int(err.argmax())
        parity = dict(rays=n_par, psnr_rgb_db=round(-10.0 * math.log10(max(mse, 1e-20)), 2),
                      psnr_rgb_db_without_worst_0p1pct=round(-10.0 * math.log10(max(mse_trim, 1e-20)), 2),
                      max_abs_rgb=round(float(err.max()), 5), rays_beyond_max_tol=int((err > PARITY_TOL["max_abs_rgb"]).sum()),
                      p99_abs_rgb=round(float(err.quantile(0.99)), 5), p999_abs_rgb=round(float(err.quantile(0.999)), 5),
                      worst_ray=dict(rgb_hip=[round(float(v), 4) for v in rgb_h[iw]], rgb_oracle=[round(float(v), 4) for v in rgb_o[iw]]),
                      precision="fp16 MFMA vs f32 oracle", tol=PARITY_TOL)
    parity["ok"] = bool(parity["psnr_rgb_db_without_worst_0p1pct"] >= PARITY_TOL["min_psnr_db"]
                        and parity["p99_abs_rgb"] <= PARITY_TOL["p99_abs_rgb"] and parity["p999_abs_rgb"] <= PARITY_TOL["p999_abs_rgb"]
                        and parity["rays_beyond_max_tol"] <= max(1, int(0.001 * n_par)))
    return parity


def time_steps(tr, steps, warmup, it):
    """ms per step of ``steps`` iterations after ``warmup`` untimed ones (device-synchronised on both sides)."""
    sync = torch.cuda.synchronize if tr.model.device.type == "cuda" else (lambda: None)
    # the cyclic collector is parked over the timed steps, as in ``timed_run`` (a generation-2 pass over torch's module
    # graphs costs tens of ms: one of them inside a 12-step variant reads as +5 ms per step); NSIM_BENCH_GC=1 leaves it on.
    # The collection runs BEFORE the warm-up steps (in front of the timed ones it left the GPU idle and clocking down).
    import gc
    park = os.environ.get("NSIM_BENCH_GC") != "1" and gc.isenabled()
    if park:
        gc.collect()
        gc.disable()
    for _ in range(warmup):
        tr.train_step(it)
        it += 1
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.train_step(it)
        it += 1
    sync()
    el = time.perf_counter() - t0
    if park:
        gc.enable()
    return el / steps * 1e3, it


FIRST_TIMED_IT = 257       # the timed region starts right after an occupancy refresh (every 16 iterations)

# --dump-outputs: arrays of more elements than this are written as a fixed, seeded sample of their entries (the same indices on
# every run of the same configuration), so that the files of one run stay within a few MB
DUMP_SAMPLE = 1 << 18
DUMP_MAX_BYTES = 64 << 20


def step_outputs(tr, loss) -> dict:
    """What a caller of the timed path holds after a step: the loss ``train_step`` returned, every parameter the step's
    optimizer update wrote (the f32 master values), the gradient that update applied, and the occupancy values the step's
    refreshes keep.  -> {name: float32 numpy array}, large arrays sampled (DUMP_SAMPLE)."""
    names = {id(tr.appear): "appear"}
    for prefix, mod in (("", tr.model), ("distant_", getattr(tr, "distant_model", None)), ("sky_", getattr(tr, "sky_model", None))):
        if mod is not None:
            names.update({id(p): prefix + n.replace(".", "_") for n, p in mod.named_parameters()})

    def host(t):
        flat = t.detach().reshape(-1)
        if flat.numel() > DUMP_SAMPLE:
            idx = torch.randint(0, flat.numel(), (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(0)).sort().values
            flat = flat[idx.to(flat.device)]
        return flat.float().cpu().numpy()

    out = {"loss": host(loss.reshape(1))}
    for i, g in enumerate(tr.optim.groups):
        p = g["p"]
        name = names.get(id(p), f"group{i}")
        if name in out:
            name = f"{name}_group{i}"
        out[name] = host(p)
        if p.grad is not None:
            out["grad_" + name] = host(p.grad)
    occ = getattr(getattr(tr.model, "accel", None), "occ_val", None)
    if occ is not None:
        out["occ_val"] = host(occ)
    assert sum(a.nbytes for a in out.values()) <= DUMP_MAX_BYTES
    return out


def dump_step_outputs(make_trainer, steps: int, rank: int, dirname: str):
    """--dump-outputs: one step of the timed path (``train_step`` at the iteration number of the last timed step) on a trainer
    built afresh by ``make_trainer`` -- the same arguments and seeds as the timed one, i.e. the state the run started from --,
    run after the timed steps, outside the timed region; rank 0 writes ``step_outputs`` of it to ``dirname``.  As in every timed
    step, its batch is prefetched on the trainer's side stream and handed over by event.
    Not the state the timed steps left behind: their gradients are summed with float atomics, whose rounding depends on the order
    the contributions arrive in, and Adam (near-zero gradients become full steps) and the occupancy thresholds grow it step by
    step.  Measured on an MI355X, two runs from the same seeded state differ after the last of N steps by (worst array, relative):
    N = 1: 2e-7, 2: 1e-4, 4: 4e-3, 8: 0.3.  One step from a fixed state is the only step whose outputs agree from run to run up to
    rounding, so that two builds can be compared output for output.  Every rank takes part (the step's collectives)."""
    tr = make_trainer()
    if getattr(tr, "pipeline", False):
        tr._prefetch()
    loss = tr.train_step(FIRST_TIMED_IT + steps - 1)
    if tr.model.device.type == "cuda":
        torch.cuda.synchronize()
    if rank == 0:
        write_outputs(step_outputs(tr, loss), dirname)
    del tr
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def write_outputs(outputs: dict, dirname: str):
    import numpy as np
    d = Path(dirname)
    d.mkdir(parents=True, exist_ok=True)
    for name, arr in outputs.items():
        np.save(d / f"{name}.npy", np.ascontiguousarray(arr, dtype=np.float32))


def measure_exposed_allreduce(tr, out, steps, it, rank, dev):
    """N > 1: the same steps with the collectives skipped (every rank keeps its local gradients and occupancy values); the
    difference to ``ms_per_step`` is the all-reduce time the overlap could NOT hide.  Replicas diverge from here on --
    the measurement is over.  Every rank calls this; rank 0's record gets the two numbers."""
    import torch.distributed as dist
    tr.skip_allreduce = True
    dist.barrier()
    ms_local, it = time_steps(tr, steps, 2, it)
    el = torch.tensor([ms_local], dtype=torch.float64, device=dev)
    dist.all_reduce(el, op=dist.ReduceOp.MAX)
    tr.skip_allreduce = False
    if rank == 0:
        out["exposed_allreduce_ms"] = round(out["ms_per_step"] - float(el.item()), 4)
        out["ms_per_step_without_allreduce"] = round(float(el.item()), 4)
    return it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline as well: the fp16-vs-oracle rendering check, the side measurements "
                         "(variants), the CPU baseline, the per-kernel table of an instrumented pass after the timed steps and, "
                         "N > 1, the exposed all-reduce leg.  A plain run sets up, warms up, times the steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what one step of the timed path computes from the state the run started "
                         "from, at the last timed iteration (its loss, the updated parameters, their gradients, the occupancy "
                         "values; large arrays as a fixed seeded sample) as DIR/<name>.npy, float32")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-variants", action="store_true", help="--full without the API-path / distant-model side measurements")
    ap.add_argument("--no-parity", action="store_true", help="--full without the fp16-vs-oracle rendering check")
    ap.add_argument("--rays-per-gpu", type=int, default=None,
                    help="rays per iteration per GPU (8192 = BASELINE configs[1]; the 4- and 8-GPU BASELINE configs draw "
                         "16384 per GPU: 65536 / 4, 131072 / 8)")
    ap.add_argument("--config", default="object", choices=("object", "street", "indoor", "multi"),
                    help="object = BASELINE configs[1] (the metric's workload, default); street / indoor / multi = the shapes of "
                         "configs[3] / [2] / [4] (neuralsim_amd/scenarios.py; 16384 rays per GPU unless --rays-per-gpu is given) -- "
                         "what the 4- / 8-GPU BASELINE configs run per GPU")
    ap.add_argument("--distant", action="store_true",
                    help="add the NeRF++ distant-view model (64 shells on every ray), as in the reference's full config")
    ap.add_argument("--sky", action="store_true", help="add the sky MLP (SimpleSky, street configs) blended per ray")
    ap.add_argument("--sdf-depth", type=int, default=2, choices=(1, 2),
                    help="hidden layers of the SDF decoder: 2 = BASELINE configs[1] (2x64, the default), 1 = the reference "
                         "yaml's own decoder_cfg D: 1 (lotd_neus.dtu.230814.yaml:120)")
    ap.add_argument("--allreduce", default=None, choices=("ring", "direct"),
                    help="N > 1: schedule of the gradient all-reduce -- ring = the backend's (RCCL) all-reduce, direct = all-to-all + "
                         "f32 reduction + all-gather (one rounding per contribution on the 2-byte wire; self-checked against "
                         "the ring on first use and abandoned with a warning if it disagrees).  Default: direct for the bf16 wire.")
    ap.add_argument("--emulator", action="store_true",
                    help="TEST HARNESS ONLY (tests/test_distributed.py drives this CLI with it): run a tiny model on the host "
                         "SIMT emulator of tests/emu over gloo instead of the HIP library over RCCL -- checks how --gpus becomes "
                         "ranks on a machine without a GPU; the line it prints says so and is not a measurement")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1")
    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(args.gpus, sys.argv[1:], emulator=args.emulator))      # becomes N ranks; never returns here
    env_world = int(os.environ.get("WORLD_SIZE", "1"))
    if env_world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher environment holds WORLD_SIZE={env_world}: the line would "
                         f"report a rank count the command did not ask for (run `python bench.py --gpus N`, or "
                         f"`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N`)")

    from neuralsim_amd import _lib, distributed as ndist
    if args.emulator:
        return main_emulator(args)
    assert torch.cuda.is_available(), "bench.py needs a HIP device (there is no CPU path)"
    if args.allreduce is not None:
        os.environ["NSIM_ALLREDUCE_ALGO"] = "ring" if args.allreduce == "ring" else ""      # "" = default rule + self-check
        if args.allreduce == "direct":
            os.environ.pop("NSIM_ALLREDUCE_ALGO")
    rank, local_rank, world = ndist.init_env()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    _lib.get_lib()
    if args.rays_per_gpu is None:
        args.rays_per_gpu = RAYS_PER_GPU if args.config == "object" else 16384
    if args.config == "object":
        def make_trainer():
            return build_trainer(dev, rank, world, distant=args.distant, sky=args.sky, sdf_D=args.sdf_depth,
                                 rays_per_gpu=args.rays_per_gpu)
        workload = None
    else:
        def make_trainer():
            return build_config_trainer(args.config, dev, rank, world, args.rays_per_gpu)
        workload = WORKLOADS[args.config]
    tr = make_trainer()
    out, it = timed_run(tr, args.steps, args.warmup, rank, world, dev, rays_per_gpu=args.rays_per_gpu, workload=workload,
                        kernel_table=args.full)
    if args.dump_outputs:
        dump_step_outputs(make_trainer, args.steps, rank, args.dump_outputs)
    if world > 1 and args.full:
        it = measure_exposed_allreduce(tr, out, min(args.steps, 32), it, rank, dev)
    dist_info = distributed_info(world, dev)         # (collective on N > 1: every rank calls it)
    if rank == 0:
        out["distributed"] = dist_info
        check_rank_count(out, args.gpus)
    if rank == 0 and args.config != "object":
        out["config"]["name"] = args.config
        out["config"]["launch_chain"] = "autograd"
        # N > 1: the tables leave during the backward, one model's exchange under the next model's kernels
        out["config"]["gradient_exchange"] = ("backward hooks (ndist.BackwardReducer)" if os.environ.get("NSIM_OVERLAP_ALLREDUCE", "1") == "1"
                                              else "after the backward")
        print(json.dumps(out), flush=True)
    elif rank == 0:
        out["config"]["distant_model"] = bool(args.distant)
        out["config"]["sky_model"] = bool(args.sky)
        out["config"]["sdf_mlp"] = f"{args.sdf_depth}x64"
        out["config"]["launch_chain"] = "fused (no autograd engine)" if tr._fused_ok() else "autograd"
        plain = world == 1 and not args.distant and not args.sky and args.full
        if plain and not args.no_parity:
            # the rendering check runs on the state the headline was just measured on, before the side measurements train the
            # model further through other paths
            out["parity"] = parity_check(tr)
        if plain and not args.no_variants:
            # side measurements of the same workload, a few steps each (not `value`): the drop-in API path (renderer +
            # autograd functions instead of the fused launch chain) and the reference's full object-centric config with
            # the distant-view model on every ray (lotd_neus.dtu.230814.yaml:186-247)
            var = {}
            tr.fused_step = False
            _lib.HOST_WAIT = 0.0       # (how long the host sat in the step's one size read: > 0 means the GPU is the bound)
            _lib.CALL_COUNT = None
            var["api_path_ms"], it = time_steps(tr, 24, 6, it)
            var["api_path_host_wait_ms"] = _lib.HOST_WAIT * 1e3 / 30.0
            _lib.HOST_WAIT = None
            tr.fused_step = True
            # the OTHER sampling semantics (VERDICT r5 weak 2 / ADVICE r5): coarse + fine samples on every AABB-tested ray, the
            # reading of rounds 1-4 -- ``upsample_on_marched_only`` is a key of THIS package (absent from the reference), so the
            # line carries the step under both values of it; `value` is the default's
            mo_now = _mo(tr)
            tro = build_trainer(dev, rank, world, sdf_D=args.sdf_depth, rays_per_gpu=args.rays_per_gpu, marched_only=not mo_now)
            key = "marched_only_" + ("false" if mo_now else "true")
            var[key + "_ms"], _ = time_steps(tro, 32, 16, 257)
            stats_o = dict(tro.stats)
            del tro
            torch.cuda.empty_cache()
            # a sharp surface (a second run at inv_s = 2000 -- late training; the default holds inv_s at e^5 = 148):
            # the fine stages concentrate their draws, the alpha mass sits in fewer samples per ray
            trs = build_trainer(dev, rank, world, sdf_D=args.sdf_depth, rays_per_gpu=args.rays_per_gpu,
                                ln_inv_s_init=math.log(2000.0) / 10.0)
            var["inv_s_2000_ms"], _ = time_steps(trs, 32, 16, 257)
            stats_s = dict(trs.stats)
            del trs
            torch.cuda.empty_cache()
            trd = build_trainer(dev, rank, world, distant=True, sdf_D=args.sdf_depth, rays_per_gpu=args.rays_per_gpu)
            var["distant_ms"], _ = time_steps(trd, 16, 8, 257)
            del trd
            torch.cuda.empty_cache()
            # the same workload on the permutohedral-lattice encoding (PermutoNeuSObj, app/models/single/neus.py:64-95;
            # SURVEY row f4): pre-trained to the sphere, stepped through the renderer + autograd path
            trp = build_trainer(dev, rank, world, sdf_D=args.sdf_depth, rays_per_gpu=args.rays_per_gpu, encoding="permuto")
            var["permuto_ms"], _ = time_steps(trp, 16, 8, 257)
            var["permuto_samples_per_hit_ray"] = round(trp.stats["S_f"] / max(1, trp.stats["R_hit"]), 1)
            del trp
            torch.cuda.empty_cache()
            # the other BASELINE configurations at their per-GPU shapes (configs[3] / [2] / [4]: 16384 rays), a few steps
            # each; their oracle parity is tests/test_fullsize_configs.py
            for name in ("street", "indoor", "multi"):
                trc = build_config_trainer(name, dev, rank, world, 16384)
                for _ in range(6):
                    trc.train_step(251)
                _lib.CALL_COUNT = 0
                var[name + "_ms"], _ = time_steps(trc, 12, 0, 257)
                # C-ABI entry-point calls of this package per step (the ATen launches of the renderer mirrors' glue are on top)
                var[name + "_abi_calls_per_step"] = round(_lib.CALL_COUNT / 12.0, 1)
                _lib.CALL_COUNT = None
                var[name + "_samples_per_hit_ray"] = round(trc.stats["S_f"] / max(1, trc.stats["R_hit"]), 1)
                del trc
                torch.cuda.empty_cache()
            # the reference's own street iteration: 8192 pixel rays + 8192 lidar beams (with_rgb=False), two optimizer
            # steps (withmask_withlidar_joint.240219.yaml:7-8; code_single/tools/train.py:1480-1590)
            from neuralsim_amd import scenarios as sc_
            trc = sc_.build_street_trainer(dev, rank, world, rays_per_gpu=8192, lidar_rays=8192)
            var["street_px8192_lidar8192_ms"], _ = time_steps(trc, 12, 6, 257)
            del trc
            torch.cuda.empty_cache()
            # a full 800 x 800 evaluation view (code_single/tools/eval.py:241-316: rayschunk pieces, validation renderer
            # settings), timed, and its PSNR against the analytic image the model is being trained on
            from neuralsim_amd.eval import psnr, render_image
            from neuralsim_amd.graphics.cameras import pinhole_selected_rays
            from neuralsim_amd.eval import all_pixel_xy
            ha = tr.appear.detach()[0:1]
            render_image(tr.renderer, tr.model, tr.intr, tr.c2w, tr.WH, frame=0, rays_h_appear=ha)       # warm-up
            ev = []
            for _ in range(3):          # (a host-paced sequence of rayschunk pieces: the median of three views)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                img = render_image(tr.renderer, tr.model, tr.intr, tr.c2w, tr.WH, frame=0, rays_h_appear=ha)
                torch.cuda.synchronize()
                ev.append((time.perf_counter() - t0) * 1e3)
            var["eval_800x800_ms"] = sorted(ev)[1]
            W_, H_ = int(tr.WH[0, 0]), int(tr.WH[0, 1])
            xy = all_pixel_xy(W_, H_, dev)
            o_, d_ = pinhole_selected_rays(xy, torch.zeros(xy.shape[0], dtype=torch.long, device=dev), tr.intr, tr.c2w, tr.WH)
            gt_img = tr.sphere_image(o_, d_, SPHERE_RADIUS).view(H_, W_, 3)
            eval_psnr = psnr(img["rgb_volume"], gt_img)
            var = {k: round(v, 3) for k, v in var.items()}
            # training converges to the target on held-out views (the fused chain's own run; the oracle-matched small-size run is
            # tests/test_convergence.py, recorded in profiles/round6_matched_psnr_small.json)
            var["convergence"] = convergence_record(dev, rank, world, sdf_D=args.sdf_depth)
            var["eval_800x800_rays_per_s"] = round(W_ * H_ / var["eval_800x800_ms"] * 1e3, 1)
            var["eval_psnr_vs_target_db"] = round(eval_psnr, 2)
            var[key + "_rays_per_s"] = round(args.rays_per_gpu / var[key + "_ms"] * 1e3, 1)
            var[key + "_S_q_per_step"], var[key + "_S_f_per_step"] = int(stats_o.get("S_q", 0)), int(stats_o.get("S_f", 0))
            var["inv_s_2000_rays_per_s"] = round(args.rays_per_gpu / var["inv_s_2000_ms"] * 1e3, 1)
            var["inv_s_2000_S_q_per_step"], var["inv_s_2000_S_f_per_step"] = int(stats_s.get("S_q", 0)), int(stats_s.get("S_f", 0))
            var["inv_s_2000_samples_per_marched_ray"] = round(stats_s.get("S_f", 0) / max(1, stats_s.get("R_live", 0)), 1)
            var["api_path_rays_per_s"] = round(args.rays_per_gpu / var["api_path_ms"] * 1e3, 1)
            var["distant_rays_per_s"] = round(args.rays_per_gpu / var["distant_ms"] * 1e3, 1)
            for name in ("street", "indoor", "multi"):
                var[name + "_rays_per_s"] = round(16384 / var[name + "_ms"] * 1e3, 1)
            out["variants"] = var
            # the reference's FULL object-centric config has the distant-view model on every ray
            # (lotd_neus.dtu.230814.yaml:186-247); BASELINE configs[1] names the hash-grid NeuS only -> `value` is without it
            out["with_distant_model"] = dict(value=var["distant_rays_per_s"], unit="rays/s", ms_per_step=var["distant_ms"],
                                             steps=16, note="same workload + NeRF++ distant model (64 shells on every ray)")
        if plain and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(tr)
        print(json.dumps(out), flush=True)
        if plain and not args.no_parity and not out["parity"]["ok"]:
            raise SystemExit(f"bench.py: fp16 rendering left the stated tolerance vs the oracle: {out['parity']}")
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


def launch_ranks(n: int, argv, emulator: bool = False) -> int:
    """``python bench.py --gpus N`` outside a launcher: become N ranks.  Re-executes this file under
    ``python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port <free>`` (the
    command shape the driver itself uses for N > 1; one rank per GPU, RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the
    launcher) with the same arguments, and returns the launcher's exit code -- rank 0 of the child prints the JSON line.
    Refuses (non-zero) when the node has fewer than N devices: N ranks on fewer GPUs would not be an N-GPU number."""
    import socket
    import subprocess
    if not emulator:
        have = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if have < n:
            print(f"bench.py: --gpus {n} asked for, {have} HIP device(s) visible on this node", file=sys.stderr)
            return 2
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(Path(__file__).resolve())] + list(argv)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // n)))
    return subprocess.call(cmd, env=env)


def check_rank_count(out: dict, gpus: int):
    """The line must describe the run that was asked for: ``n_gpus`` == ``--gpus`` == the ranks the process group reported.
    (Round 4's ``--gpus 8`` without a launcher ran ONE rank and printed n_gpus 1.)"""
    seen = out["distributed"]["ranks_seen"]
    if not (out["n_gpus"] == gpus == seen):
        raise SystemExit(f"bench.py: rank count mismatch: --gpus {gpus}, n_gpus {out['n_gpus']}, process group reports {seen}")


def main_emulator(args):
    """``--emulator``: the N-rank control flow of this file on a machine without a GPU (test harness; the product has no CPU
    path -- the emulator library lives under tests/emu and is injected here exactly as tests/conftest.py injects it)."""
    import ctypes
    sys.path.insert(0, str(ROOT / "tests"))
    sys.path.insert(0, str(ROOT / "tests" / "emu"))
    import build_emu
    from neuralsim_amd import _lib, distributed as ndist
    lib = _lib.bind(ctypes.CDLL(str(build_emu.build())))
    _lib.get_lib = lambda: lib
    _lib.stream_handle = lambda: 0
    _lib.require_device = lambda t, name="tensor": None
    torch.set_num_threads(2)
    torch.manual_seed(0)
    rank, local_rank, world = ndist.init_env(backend="gloo", device_type="cpu")
    dev = torch.device("cpu")
    from test_trainer import _tiny
    from neuralsim_amd.graphics.cameras import look_at_cameras
    from neuralsim_amd.trainer import RenderTrainer
    m = _tiny(dev, seed=42 + rank)                       # replicas differ until the broadcast
    ndist.broadcast_module(m)
    intr, c2w, WH = look_at_cameras(V=4, seed=1, device=dev)
    rays = int(args.rays_per_gpu or 16)

    def make_trainer():
        m_ = _tiny(dev, seed=42 + rank)
        ndist.broadcast_module(m_)
        return RenderTrainer(m_, intr, c2w, WH, num_rays=rays, lr=1e-3, num_uniform=16, rank=rank, world_size=world)
    tr = RenderTrainer(m, intr, c2w, WH, num_rays=rays, lr=1e-3, num_uniform=16, rank=rank, world_size=world)
    out, it = timed_run(tr, args.steps, args.warmup, rank, world, dev, rays_per_gpu=rays, kernel_table=args.full)
    if args.dump_outputs:
        dump_step_outputs(make_trainer, args.steps, rank, args.dump_outputs)
    import torch.distributed as dist
    if world > 1:          # replicas agree after the all-reduced updates (asserted on every rank) ...
        w = m.sdf_w.detach().clone()
        ws = [torch.zeros_like(w) for _ in range(world)]
        dist.all_gather(ws, w)
        assert all(torch.equal(ws[0], x) for x in ws[1:]), "replicas diverged"
        if args.full:
            it = measure_exposed_allreduce(tr, out, min(args.steps, 2), it, rank, dev)      # ... and diverge from here on
    dist_info = distributed_info(world, dev)
    if rank == 0:
        out["distributed"] = dist_info
        out["data"] = "synthetic (HOST EMULATOR of the kernels, tiny model: control-flow check, NOT a measurement)"
        out["emulator"] = True
        check_rank_count(out, args.gpus)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def distributed_info(world: int, dev) -> dict:
    """What the N > 1 run actually was (recorded in the line so that a scaling number can be checked against it): ranks the
    process group reports, every rank's device, backend, the all-reduce schedule that ended up in use and the wire dtype."""
    import torch.distributed as dist
    from neuralsim_amd import distributed as ndist
    name = torch.cuda.get_device_name(dev) if dev.type == "cuda" else "cpu"
    info = dict(ranks_seen=1, devices=[f"{dev}: {name}"], backend=None, allreduce=None, wire_dtype=None)
    if world > 1 and dist.is_initialized():
        names = [None] * dist.get_world_size()
        dist.all_gather_object(names, f"rank {dist.get_rank()} {dev}: {name}")
        wire = ndist.wire_dtype_default()
        algo = ndist._algo(wire)
        if algo == "direct" and not ndist._DIRECT_OK.get((dist.get_backend(), str(dev)), True):
            algo = "ring (direct failed its self-check)"
        info.update(ranks_seen=dist.get_world_size(), devices=names, backend=dist.get_backend(), allreduce=algo,
                    wire_dtype=str(wire).replace("torch.", ""))
    return info


WORKLOADS = {
    "street": "BASELINE configs[3] shape: StreetSurf street view (synthetic 6-camera rig on a 200 x 100 x 30 m analytic street), "
              "{rays} rays/iter/GPU, cuboid 19-level LoTD (T=2^20, ~33 Mi params) + 1x64 SDF MLP (sdf_scale 25) + 2x64 radiance, occ grid "
              "200x100x30 (1 m voxels), num_coarse 128, num_fine [8,8,32], step .2, upsample_use_estimate_alpha false, compressed query, "
              "distant NeRF++ model (64 cuboid shells, 16 Mi 4-D table, no view dirs) + sky MLP, l1 photometric + eikonal on render samples "
              "and 2^16 uniform points, Adam + occupancy refresh inside the timed region",
    "indoor": "BASELINE configs[2] shape: MonoSDF indoor (synthetic box room seen from inside, inside_out), {rays} rays/iter/GPU = 64x64 image "
              "patch + pixel rays, L=16 hashgrid (T=2^19) + 2x64 SDF MLP + 2x64 radiance, normals + depth rendered with gradient, losses "
              "mse + eikonal + mono normal (l1 + cos) + scale-shift-invariant mono depth on the patch, Adam + occupancy refresh",
    "multi": "BASELINE configs[4] shape: code_multi scene graph -- street background (as configs[3]) + 8 posed instances of one shared "
             "batched vehicle model (8 dense levels 5..144, per-instance tables, batched occ grid 8x32^3, num_coarse 32, num_fine [8,8]) + "
             "distant + sky through the BufferComposeRenderer mirror, {rays} rays/iter/GPU, l1 photometric + eikonal, Adam on every model",
}


def build_config_trainer(name, dev, rank, world, rays_per_gpu, precision="fp16"):
    """Trainer of one BASELINE configuration: "object" = configs[1] (the metric's), "street" / "indoor" / "multi" = the
    shapes of configs[3] / [2] / [4] (neuralsim_amd/scenarios.py)."""
    from neuralsim_amd import scenarios as sc
    if name == "street":
        return sc.build_street_trainer(dev, rank, world, precision=precision, rays_per_gpu=rays_per_gpu)
    if name == "indoor":
        return sc.build_indoor_trainer(dev, rank, world, precision=precision, rays_per_gpu=rays_per_gpu)
    if name == "multi":
        return sc.build_multi_trainer(dev, rank, world, precision=precision, rays_per_gpu=rays_per_gpu)
    raise ValueError(name)


def _mo(tr) -> bool:
    from neuralsim_amd.fields.neus import marched_only
    return bool(marched_only(tr.model.ray_query_cfg.get("query_param", {})))


def timed_run(tr, steps, warmup, rank, world, dev, rays_per_gpu, workload=None, kernel_table=True):
    """W untimed warm-up steps, then exactly K steps bracketed by barrier + device sync on both sides; the elapsed
    time is the MAX over ranks; rank 0 returns the JSON record (other ranks None) and the next iteration number.
    ``kernel_table``: the per-kernel table from an instrumented pass of its own after the timed steps (bench.py --full)."""
    from neuralsim_amd import _lib
    import torch.distributed as dist
    on_gpu = dev.type == "cuda"
    it0 = FIRST_TIMED_IT
    it = it0 - max(warmup, 1)
    # the warm-up steps run with the same instrumentation as the timed ones (HIP-event pairs around the modelled entry points:
    # their first creations are slow), so the first timed step does not pay for the bench's own timer
    dm_w = getattr(tr, "distant_model", None) or getattr(tr, "distant", None)
    if on_gpu and os.environ.get("NSIM_BENCH_WARM_TIMER", "1") == "1":
        _lib.TIMER = _lib.KernelTimer(only=kernel_model(tr.model.encoding.cfg.num_levels,
                                                        dm_w.cfg.num_levels if dm_w is not None else 12).keys())
    import gc
    for w_ in range(warmup):
        if w_ == max(0, warmup - 4):
            # the cyclic collector is parked over the timed steps (a generation-2 pass over torch's module graph costs tens
            # of ms, i.e. ~10 steps); NSIM_BENCH_GC=1 leaves it on.  The collection itself runs HERE, with warm-up steps
            # still to come: done right in front of the timed region it left the GPU idle for tens of ms and the first
            # timed steps ran on a chip that was clocking back up (first step 2.5-3.0 ms instead of 1.2)
            gc.collect()
            if os.environ.get("NSIM_BENCH_GC") != "1":
                gc.freeze()
                gc.disable()
        tr.train_step(it)
        it += 1
    timer_w, _lib.TIMER = _lib.TIMER, None
    it = it0

    def fence():
        if world > 1:
            dist.barrier()
        if on_gpu:
            torch.cuda.synchronize()

    if warmup == 0:
        gc.collect()
        if os.environ.get("NSIM_BENCH_GC") != "1":
            gc.freeze()
            gc.disable()
    fence()
    # HIP events around the modelled kernels only (on the launch stream)
    dm_ = getattr(tr, "distant_model", None) or getattr(tr, "distant", None)
    KM = kernel_model(tr.model.encoding.cfg.num_levels, dm_.cfg.num_levels if dm_ is not None else 12)
    # Inside the timed region ONLY the dominant kernel carries HIP events (the roofline's live measurement): an event pair is a
    # marker packet on either side of a launch, and the 14 pairs per step of the full per-kernel table cost the step 0.085 ms
    # (1.20 -> 1.12 ms median, measured: gpurun_out/r6_s2_trace) -- the bench was slowing down what it measures.  Which kernel
    # dominates is read from the instrumented warm-up steps; the table of all modelled kernels comes from a short instrumented
    # pass AFTER the timed region (``kernels_source`` says so).  NSIM_BENCH_KTIMER=full: every modelled kernel inside, as before.
    kt_mode = os.environ.get("NSIM_BENCH_KTIMER", "1")
    dom_w = "nsim_lotd_scatter"
    if timer_w is not None and timer_w.events and warmup >= 3:
        # per entry point: launches x MEDIAN launch time over the warm-up (the first, cold launches of a short warm-up skew a mean:
        # a 5-step warm-up once put the gathers in front of the scatter); the table scatter stays unless another one clearly outweighs it
        torch.cuda.synchronize()
        tot_w = {}
        for k_, evs in timer_w.events.items():
            if k_ in KM and evs:
                ms_ = sorted(a_.elapsed_time(b_) for a_, b_ in evs)
                tot_w[k_] = len(ms_) * ms_[len(ms_) // 2]
        if tot_w:
            best = max(tot_w, key=tot_w.get)
            if dom_w not in tot_w or tot_w[best] > 1.15 * tot_w[dom_w]:
                dom_w = best
    only_ = KM.keys() if kt_mode == "full" else [dom_w]
    _lib.TIMER = _lib.KernelTimer(only=only_) if (on_gpu and kt_mode != "0") else None
    _lib.CALL_COUNT = 0
    _lib.HOST_WAIT = 0.0
    S_f = S_hit = S_q = S_live = 0
    marks = []
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.train_step(it)
        it += 1
        S_f += tr.stats["S_f"]
        S_hit += tr.stats["R_hit"]
        S_q += tr.stats.get("S_q", 0)
        S_live += tr.stats.get("R_live", tr.stats["R_hit"])
        marks.append(time.perf_counter() - t0)      # host side; every step blocks once on its sample count
    fence()
    elapsed = time.perf_counter() - t0
    gc.enable()
    timer, _lib.TIMER = _lib.TIMER, None
    abi_calls = _lib.CALL_COUNT
    _lib.CALL_COUNT = None
    host_wait, _lib.HOST_WAIT = _lib.HOST_WAIT, None
    el = torch.tensor([elapsed], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
    elapsed = float(el.item())

    if os.environ.get("NSIM_BENCH_TRACE") and rank == 0:
        prev = 0.0
        for i in range(0, len(marks), 8):
            chunk = marks[i:i + 8]
            print(f"[trace] steps {i}-{i + len(chunk) - 1}: {(chunk[-1] - prev) / len(chunk) * 1e3:.3f} ms/step", file=sys.stderr)
            prev = chunk[-1]
        if os.environ.get("NSIM_BENCH_TRACE") == "2":       # every step (host-side marks: each step blocks once)
            d = [marks[0]] + [b - a for a, b in zip(marks, marks[1:])]
            print("[trace] per step ms: " + " ".join(f"{x * 1e3:.2f}" for x in d), file=sys.stderr)
    # the per-kernel table: a short pass with every modelled entry point instrumented, outside the timed region (all ranks)
    n_post = 0
    ksum_post = {}
    if timer is not None and kt_mode != "full" and kernel_table:
        n_post = max(1, min(16, steps))
        _lib.TIMER = _lib.KernelTimer(only=KM.keys())
        for _ in range(n_post):
            tr.train_step(it)
            it += 1
        fence()
        tp, _lib.TIMER = _lib.TIMER, None
        ksum_post = tp.summary()
    if rank != 0:
        return None, it
    ksum = timer.summary() if timer is not None else {}
    for k_, v_ in ksum_post.items():      # (the dominant kernel keeps its timed-region measurement)
        ksum.setdefault(k_, v_)
    total_rays = rays_per_gpu * world * steps
    ms = elapsed / steps * 1e3
    if not ksum:
        return dict(metric="training rays/sec (fwd+bwd) NeuS 800x800", value=round(total_rays / elapsed, 1),
                    unit="rays/s", n_gpus=world, steps=steps, warmup=warmup, ms_per_step=round(ms, 3),
                    higher_is_better=True, scaling="weak", vs_baseline=None, dtype="fp16", data="synthetic",
                    config=dict(workload="emulator smoke run"), roofline=None), it
    # the roofline's kernel: the one that carried events inside the timed region (the other entries of ``ksum`` come from the post
    # pass: other call counts, their totals do not compare)
    dom = dom_w if (kt_mode != "full" and dom_w in ksum) else max((k for k in ksum if k in KM), key=lambda k: ksum[k]["total_ms"])
    kd = ksum[dom]
    bound, per_pt = KM[dom]
    work_per_launch = kd["units"] * per_pt / max(1, kd["calls"])
    if bound == "hbm":
        achieved, peak, unit = work_per_launch / (kd["avg_ms"] * 1e-3) / 1e9, HBM_PEAK_GBS, "GB/s"
    else:
        achieved, peak, unit = work_per_launch / (kd["avg_ms"] * 1e-3) / 1e12, MFMA_PEAK_TFLOPS, "TFLOP/s"
    roofline = dict(bound=bound, kernel=dom, achieved=round(achieved, 3), peak=peak, unit=unit,
                    frac=round(achieved / peak, 5), traffic=None, avg_launch_ms=round(kd["avg_ms"], 4),
                    points_per_launch=kd["units"] / max(1, kd["calls"]), work_per_point=per_pt)
    if bound == "hbm":
        # the same rate against the copy bandwidth measured on this chip (MI355X_MICROARCH.md: 6.29 TB/s) next to the 8 TB/s spec
        roofline["frac_of_measured_copy_6290GBs"] = round(achieved / 6290.0, 5)
    tf = ROOT / "profiles" / "traffic.json"      # per-launch HBM bytes from rocprofv3 PMC passes (FETCH_SIZE + WRITE_SIZE)
    if tf.exists() and workload is None:
        try:
            rec_t = json.loads(tf.read_text())
            roofline["traffic"] = rec_t.get(dom)
            roofline["traffic_source"] = ("profiles/traffic.json: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this "
                                          "bench command, recorded " + str(rec_t.get("_recorded", "in an earlier profiling "
                                          "run")) + " -- NOT collected by the run that prints this line")
        except Exception:
            pass
    # The ceilings that actually bind the two largest kernels sit between L1 and L2, not at HBM: the random 4-byte gather is
    # limited by the TCP -> TCC request rate (one 128-byte line per distinct line touched), the gradient scatter by the rate
    # of atomic requests; both ceilings are measured by micro-benchmarks on this chip, the kernels' request counts by PMC
    # passes of this command (profiles/round4_l2_requests.json -- recorded, NOT collected by the run that prints this line)
    lf = ROOT / "profiles" / "l2_requests.json"
    if not lf.exists():
        lf = ROOT / "profiles" / "round4_l2_requests.json"
    if lf.exists() and workload is None:
        try:
            rec_l = json.loads(lf.read_text())
            kk = rec_l["kernels"]
            # (kernel names as rocprofv3 prints them: the scatter became a template in round 6)
            ga = next(v for k, v in kk.items() if "k_lotd_gather_lm<1, false>" in k)
            sc_ = next(v for k, v in kk.items() if "k_lotd_scatter" in k)
            roofline["cache_ceilings"] = dict(
                gather=dict(kernel="k_lotd_gather_lm<1,false>", read_req_per_launch=ga["tcp_tcc_read_req"],
                            achieved_Greq_s=ga["read_req_per_s"], ceiling_Greq_s=rec_l["calibration"]["l2_read_req_ceiling_per_s"] / 1e9,
                            frac=ga["frac_of_l2_read_req_ceiling"]),
                scatter=dict(kernel="k_lotd_scatter", atomic_req_per_launch=sc_["atomic_req"],
                             achieved_Greq_s=sc_["atomic_req_per_s_G"], ceiling_Greq_s=rec_l["calibration"]["atomic_req_ceiling_per_s"] / 1e9,
                             frac=sc_["frac_of_atomic_req_ceiling"]),
                source=f"profiles/{lf.name} (rocprofv3 --pmc TCP_TCC_READ_REQ_sum / TCP_TCC_ATOMIC_WITHOUT_RET_REQ_sum passes of this "
                       f"command + tools/gather_pair_bench, tools/atomic_bench4), recorded {rec_l.get('_recorded', 'round 4')} -- NOT "
                       "collected by the run that prints this line")
        except Exception:
            pass
    # The MFMA kernels against the ceiling of their own CHAIN (round 5): tools/decoder_chain_bench.hip runs the 32 -> 64 -> 64 -> 1
    # chains -- the same products and softplus / sigmoid evaluations -- on register-resident tiles, no planes, no LDS staging
    # (profiles/round5_decoder_chain_bench.txt: G points/s chip-wide, best of 1 / 2 / 4 waves per SIMD and both tile shapes);
    # recorded, NOT measured by the run that prints this line.  A 64-wide softplus network tops out at 12-23 % of the dense
    # f16 MFMA peak on this chip; `frac_of_chain_ceiling` = the product kernel's points/s over that ceiling
    CHAIN_CEIL = {"nsim_field_sdf": ("forward (sdf query); the product runs it in split precision: 3 MFMAs per product", 24.67e9),
                  "nsim_field_fwd": ("forward + d sdf / d h (+ the level-major gather and the radiance forward in the same entry point)", 17.17e9),
                  "nsim_field_bwd_sdf": ("2nd-order backward chain + weight-gradient MFMAs", 7.88e9)}
    chain = {}
    for k, (what, ceil_pts) in CHAIN_CEIL.items():
        v = ksum.get(k)
        if v and v["units"] and v["total_ms"] > 0 and workload is None:
            pts_s = v["units"] / (v["total_ms"] * 1e-3)
            chain[k] = dict(chain=what, ceiling_Gpts_s=round(ceil_pts / 1e9, 2), achieved_Gpts_s=round(pts_s / 1e9, 3),
                            frac_of_chain_ceiling=round(pts_s / ceil_pts, 4))
    ks = ROOT / "profiles" / "kernel_split.json"       # recorded: the decoder kernel's share of the nsim_field_fwd entry point
    if "nsim_field_fwd" in chain and ks.exists():
        sp = json.loads(ks.read_text())
        f_ = sp["nsim_field_fwd"]
        share = f_["decoder_avg_us"] / (f_["decoder_avg_us"] + f_["gather_avg_us"])
        c_ = chain["nsim_field_fwd"]
        c_["decoder_kernel_alone"] = dict(share_of_entry_point_time=round(share, 3),
                                          achieved_Gpts_s=round(c_["achieved_Gpts_s"] / share, 3),
                                          frac_of_chain_ceiling=round(c_["frac_of_chain_ceiling"] / share, 4),
                                          note="the entry point's HIP-event time x the decoder kernel's share of it in the rocprofv3 "
                                               "kernel trace (its level-major gather is the other kernel); the radiance forward is part "
                                               "of the decoder kernel and not of the chain", source="profiles/kernel_split.json: " + sp.get("_recorded", ""))
    if chain:
        roofline["chain_ceilings"] = dict(kernels=chain, source="profiles/round5_decoder_chain_bench.txt (tools/decoder_chain_bench.hip on MI355X), recorded")
    # per-kernel roofline of every modelled entry point (the MFMA kernels against the dense fp16 peak)
    per_kernel = {}
    for k, v in sorted(ksum.items(), key=lambda kv: -kv[1]["total_ms"]):
        if k not in KM or not v["calls"] or not v["units"]:
            continue
        b_, w_ = KM[k]
        rate = v["units"] * w_ / (v["total_ms"] * 1e-3)
        per_kernel[k] = dict(calls=v["calls"], total_ms=round(v["total_ms"], 3), avg_ms=round(v["avg_ms"], 4), bound=b_,
                             frac=round(rate / (HBM_PEAK_GBS * 1e9 if b_ == "hbm" else MFMA_PEAK_TFLOPS * 1e12), 5))
    d = sorted(b - a for a, b in zip([0.0] + marks[:-1], marks))
    q = lambda f: round(d[min(len(d) - 1, int(f * len(d)))] * 1e3, 3)       # noqa: E731
    out = dict(metric="training rays/sec (fwd+bwd) NeuS 800x800", value=round(total_rays / elapsed, 1),
               unit="rays/s", n_gpus=world, steps=steps, warmup=warmup, ms_per_step=round(ms, 3),
               higher_is_better=True, scaling="weak", vs_baseline=None, dtype="fp16", data="synthetic",
               config=dict(workload=workload.format(rays=rays_per_gpu) if workload else
                           "BASELINE configs[1]: NeuS single object (DTU scan24-style synthetic), "
                                    f"{rays_per_gpu} rays/iter/GPU, L=16 hashgrid (T=2^19, F=2) + {tr.model.sdf_D}x64 SDF MLP + 2x64 radiance "
                                    "MLP (SH4, appear 4), synthetic sphere r=0.75 (~40% coverage) supervised by its analytic image, occ grid 64^3, num_coarse 64, "
                                    "num_fine [8,8,32], "
                                    f"step .005, query_mode march_occ_multi_upsample_compressed (reference default), upsample_on_marched_only "
                                    f"{str(_mo(tr)).lower()} (coarse + fine samples on the rays whose occupancy march found something), inv_s=e^5, eikonal on "
                                    "render samples + 4096 uniform points, "
                           "Adam + occupancy refresh every 16 it inside the timed region",
                           rays_per_gpu=rays_per_gpu, parallelism=f"dp{world} (rays sharded, RCCL grad all-reduce)",
                           upsample_on_marched_only=_mo(tr),
                           adam="touched-entries tables (NSIM_LAZY_ADAM=1, opt-in: NOT the reference's optimizer)"
                           if getattr(tr.optim, "lazy_tables", False) else "dense (the reference's torch.optim.Adam rule)",
                           # realised sample statistics: rays that pass the AABB test / whose march finds occupied
                           # voxels, SDF-only queries of the sampling pass (S_q) and with-grad samples (S_f) per step
                           samples_per_hit_ray=round(S_f / max(1, S_hit), 1),
                           samples_per_marched_ray=round(S_f / max(1, S_live), 1),
                           hit_fraction=round(S_hit / (rays_per_gpu * steps), 3),
                           marched_fraction=round(S_live / (rays_per_gpu * steps), 3),
                           S_q_per_step=round(S_q / steps), S_f_per_step=round(S_f / steps)),
               # `value` / `ms_per_step` are the contract's figures: K steps / elapsed (the MEAN step, which carries the occupancy
               # refresh steps -- 4 x 2^20 queries every 16 iterations, ~3 ms each).  The MEDIAN step next to it, first-class
               # (VERDICT r4 weak #10): host-side marks, every step blocks once on its sample count
               ms_per_step_p50=q(0.5), value_p50=round(rays_per_gpu * world / max(q(0.5), 1e-9) * 1e3, 1),
               step_ms=dict(p10=q(0.1), p50=q(0.5), p90=q(0.9), max=round(d[-1] * 1e3, 3)),
               roofline=roofline, kernels=per_kernel,
               kernels_source=(f"HIP events inside the timed region for the dominant kernel ({dom}: the roofline's live measurement); the "
                               f"other entry points from {n_post} instrumented steps run right after it -- 14 event pairs per step inside "
                               "the timed region cost the step 0.085 ms (NSIM_BENCH_KTIMER=full restores them)") if n_post else
                              "HIP events inside the timed region for every modelled entry point (NSIM_BENCH_KTIMER=full)"
                              if kt_mode == "full" else
                              (f"HIP events inside the timed region for the dominant kernel ({dom}) only; the table of the other "
                               "entry points is an instrumented pass of its own after the timed steps (bench.py --full)"),
               # C-ABI entry-point calls of this package per step (each is one kernel launch, three of them two); the ATen /
               # rocprim launches of the host glue (rand, fill, cat, compaction) are on top: profiles/round4_rocprofv3_kernel_stats
               abi_calls_per_step=round(abi_calls / max(1, steps), 1) if abi_calls is not None else None,
               # host time blocked on the step's one size read: ~0 = the host (launch overhead) paces the step, not the GPU
               host_wait_ms_per_step=round(host_wait / max(1, steps) * 1e3, 4))
    return out, it


if __name__ == "__main__":
    main()
