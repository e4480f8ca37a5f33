"""Float64 CPU restatement of the scene-flow pieces of the EmerNeRF dynamic model: the position gradient of the
point-mode lattice gather (``nsim_permuto_dx_pts``), the flow decoder (``nsim_flow_fwd`` / ``_bwd``), the flow warp
(``nsim_dyn_warp_fwd`` / ``_bwd``) and the two terms of the flow loss (``nsim_flow_loss_fwd`` / ``_bwd``,
``losses.flow_loss``).  Builds on tests/dynamic_nerf_ref.py (the model without flow) and oracle/permuto.py (the lattice), both
unchanged.  Written from the stated semantics, not from the kernels.  Test infrastructure only."""
import torch

import dynamic_nerf_ref as dref          # noqa: F401  (the model this restatement extends)
from oracle import permuto as op


# ------------------------------------------------------------------------------------------------ lattice, position gradient
def active_features(x4: torch.Tensor, grid: torch.Tensor, spec: op.PermutoSpec, n_active: int = None) -> torch.Tensor:
    """Lattice features [S, 2 L] at the points x4 [S, d] (f64, may require grad); levels >= n_active give zeros and their tables
    are not touched (a NaN there must not reach the result)."""
    L = spec.num_levels
    na = L if n_active is None or n_active <= 0 or n_active >= L else n_active
    if na == L:
        return op.permuto_forward(x4, grid, spec)
    sub = op.PermutoSpec(spec.in_dim, spec.res[:na], spec.n_feats, spec.hashmap_size, spec.shifts[:na])
    feat = op.permuto_forward(x4, grid[:sub.n_params], sub)
    return torch.cat([feat, feat.new_zeros(x4.shape[0], 2 * (L - na))], dim=-1)


def dx_pts(x4: torch.Tensor, grid: torch.Tensor, spec: op.PermutoSpec, dh: torch.Tensor, n_active: int = None) -> torch.Tensor:
    """d (sum_s dh[s] . h(x4[s])) / d x4 by float64 autograd: [S, d].  dh [S, 2 L]; entries of masked levels are not read."""
    x = x4.detach().double().clone().requires_grad_(True)
    feat = active_features(x, grid.detach().double(), spec, n_active)
    L = spec.num_levels
    na = L if n_active is None or n_active <= 0 or n_active >= L else n_active
    (feat[:, :2 * na] * dh.double()[:, :2 * na]).sum().backward()
    return x.grad


def face_gap(x4: torch.Tensor, spec: op.PermutoSpec) -> torch.Tensor:
    """[S]: how close each point comes to a simplex face on any level.  The barycentric weights of a point are the gaps between
    its sorted lattice residuals (oracle.permuto.barycentric: b_k = delta_(k) - delta_(k+1), the first closing the cycle with + 1);
    a weight of 0 is a tie of two residuals, i.e. a face, where d h / d x jumps.  The smallest weight over all levels, in f64."""
    gap = torch.full([x4.shape[0]], float("inf"), dtype=torch.float64)
    for l in range(spec.num_levels):
        xs = (x4.double() + spec.shifts[l].double()) * spec.scale_factors(l).double()
        elev = op.elevate(xs)
        rem0, rank = op.simplex(elev)
        gap = torch.minimum(gap, op.barycentric(elev, rem0, rank).min(dim=1).values)
    return gap


def dx_points(S: int, seed: int) -> torch.Tensor:
    """the f32 lattice points of the position-gradient tests: [S, 4] uniform in [-1, 1]"""
    g = torch.Generator().manual_seed(1000 * seed + S)
    return torch.rand(S, 4, generator=g) * 2 - 1


def pick_dx_seed(S: int, spec: op.PermutoSpec, min_gap: float = 1e-4, cap: float = 0.02, tries: int = 64):
    """The first seed whose points leave at most ``cap`` of them within ``min_gap`` of a face -- decided by this restatement alone.
    -> (seed, x4 [S,4] f32, excluded bool [S])"""
    for seed in range(tries):
        x = dx_points(S, seed)
        excl = face_gap(x, spec) < min_gap
        if int(excl.sum()) <= int(cap * S):
            return seed, x, excl
    raise AssertionError(f"no seed below {tries} keeps the excluded share of {S} points under {cap}")


# ------------------------------------------------------------------------------------------------ flow decoder, warp
def make_flow_decoder(L: int, seed: int = 4):
    """(flow_w, flow_b) f32, flat row-major [64 x 2L | 64 x 64 | 6 x 64], [64 | 64 | 6]: uniform(+-1 / sqrt(fan-in)), as the model's
    ``lin``"""
    g = torch.Generator().manual_seed(seed)

    def lin(o, i):
        b = 1.0 / (i ** 0.5)
        return (torch.rand(o, i, generator=g) * 2 - 1) * b, (torch.rand(o, generator=g) * 2 - 1) * b
    (w1, b1), (w2, b2), (w3, b3) = lin(64, 2 * L), lin(64, 64), lin(6, 64)
    return torch.cat([w1.reshape(-1), w2.reshape(-1), w3.reshape(-1)]), torch.cat([b1, b2, b3])


def flow_decoder(h: torch.Tensor, flow_w: torch.Tensor, flow_b: torch.Tensor) -> torch.Tensor:
    """h [S, F] -> flow6 [S, 6] = W3 relu(W2 relu(W1 h + b1) + b2) + b3 (no output activation): columns 0..2 flow_fwd, 3..5
    flow_bwd.  In the tensors' precision (f64 for the tests)."""
    F = h.shape[1]
    w1, w2, w3 = flow_w[:64 * F].view(64, F), flow_w[64 * F:64 * F + 4096].view(64, 64), flow_w[64 * F + 4096:].view(6, 64)
    b1, b2, b3 = flow_b[:64], flow_b[64:128], flow_b[128:]
    a1 = torch.relu(h @ w1.t() + b1)
    a2 = torch.relu(a1 @ w2.t() + b2)
    return a2 @ w3.t() + b3


def time_neighbours(w: torch.Tensor, T: int, lo: float = -1.0, hi: float = 1.0):
    """(delta, w+, w-): delta = (hi - lo) / (T - 1) (0 for one keyframe), w+ = min(w + delta, hi), w- = max(w - delta, lo)"""
    delta = (hi - lo) / (T - 1) if T > 1 else 0.0
    return delta, (w + delta).clamp(max=hi), (w - delta).clamp(min=lo)


def warp(x4: torch.Tensor, flow6: torch.Tensor, delta: float, lo: float, hi: float) -> torch.Tensor:
    """[2S,4]: (x + flow_fwd, w+) | (x + flow_bwd, w-); x in object coordinates, not clamped to the AABB"""
    w = x4[:, 3:]
    fwd = torch.cat([x4[:, :3] + flow6[:, :3], (w + delta).clamp(max=hi)], dim=1)
    bwd = torch.cat([x4[:, :3] + flow6[:, 3:], (w - delta).clamp(min=lo)], dim=1)
    return torch.cat([fwd, bwd], dim=0)


# ------------------------------------------------------------------------------------------------ flow loss
def flow_loss(flow_fwd, flow_fwd_pred_bwd, flow_bwd, flow_bwd_pred_fwd, w_cycle=1.0, w_sparsity=1.0):
    """(w_cycle cycle, w_sparsity sparsity) of DESIGN.md sec. 7 in the tensors' own precision (f64 for the tests):
      cycle    = 1/2 mean over S 3 of (sg(flow_fwd) + flow_fwd_pred_bwd)^2 + (sg(flow_bwd) + flow_bwd_pred_fwd)^2
      sparsity = 1/4 mean over S of the four row norms (torch's norm: the gradient at a zero row is zero)"""
    cyc = 0.5 * ((flow_fwd.detach() + flow_fwd_pred_bwd) ** 2 + (flow_bwd.detach() + flow_bwd_pred_fwd) ** 2).mean()
    spa = 0.25 * (flow_fwd.norm(dim=-1) + flow_fwd_pred_bwd.norm(dim=-1) + flow_bwd.norm(dim=-1) +
                  flow_bwd_pred_fwd.norm(dim=-1)).mean()
    return w_cycle * cyc, w_sparsity * spa


# ------------------------------------------------------------------------------------------------ the ``flow`` block
FLOW_KEYS = ("flow_fwd", "flow_fwd_pred_bwd", "flow_bwd", "flow_bwd_pred_fwd")
# the block of code_multi/configs/exps/fg_emernerf/no_gtbox_with_flow.240208.yaml:664-672 with its two weights filled in
YAML_FLOW_BLOCK = dict(class_name_cfgs=dict(Dynamic=dict(cycle=dict(w=0.01, on_render_ratio=1.0),
                                                         sparsity=dict(w=0.001, on_render_ratio=0.1))))
ANNEAL = dict(type="linear", start_it=0, stop_it=100, start_val=0.0, stop_val=0.02)
# name -> (block, it): a constant w, an annealed w, per-term / per-class / module render ratios, no uniform samples, one term only
FLOW_BLOCK_CASES = {
    "yaml": (YAML_FLOW_BLOCK, 0),
    "anneal": (dict(class_name_cfgs=dict(Dynamic=dict(cycle=dict(anneal=ANNEAL), sparsity=dict(w=0.001, anneal=ANNEAL)),
                                         Pedestrian=dict(cycle=dict(w=0.5))), on_render_ratio=0.25), 37),
    "class_ratio": (dict(class_name_cfgs=dict(Dynamic=dict(cycle=dict(w=0.3), sparsity=dict(w=0.2, on_render_ratio=0.5),
                                                           on_render_ratio=0.75),
                                              Pedestrian=dict(sparsity=dict(w=1.0), on_render_ratio=0.0))), 5),
    "render_only": (dict(class_name_cfgs=dict(Dynamic=dict(cycle=dict(w=1.0)), Pedestrian=dict(sparsity=dict(w=2.0))),
                         on_uniform_samples=False, on_render_ratio=0.5), 0),
}


def flow_block_inputs(dtype=torch.float32, device=None):
    """-> (raw_per_obj_model, uniform_samples): two classes with flow tensors of different sizes, a third object of the first class
    whose buffer is ``empty`` (skipped), a class the blocks do not name.  Stand-in tensors of the sizes and magnitudes of a query's
    flow outputs (the model that emits them is not part of this package yet)."""
    g = torch.Generator().manual_seed(21)

    def four(n, s):
        return {k: (torch.randn(n, 3, generator=g) * s).to(dtype).to(device) for k in FLOW_KEYS}
    raw = dict(dyn0=dict(class_name="Dynamic", model_id="dyn0", volume_buffer=dict(type="packed", **four(333, 0.05))),
               dyn1=dict(class_name="Dynamic", model_id="dyn1", volume_buffer=dict(type="empty")),
               ped0=dict(class_name="Pedestrian", model_id="ped0", volume_buffer=dict(type="packed", **four(65, 0.2))),
               bg=dict(class_name="Street", model_id="bg", volume_buffer=dict(type="packed")))
    uni = dict(Dynamic=four(129, 0.03), Pedestrian=four(64, 0.1))
    return raw, uni


def reference_flow_terms(mod, block: dict, it: int, raw, uni) -> dict:
    """the reference's ``FlowLoss`` (``mod`` = app/loss/flow.py loaded unchanged) on one case"""
    import copy
    blk = copy.deepcopy(block)
    fn = mod.FlowLoss(blk["class_name_cfgs"], ["Dynamic", "Pedestrian"], on_uniform_samples=blk.get("on_uniform_samples", True),
                      on_render_ratio=blk.get("on_render_ratio", 1.0))
    return fn(None, dict(raw_per_obj_model=raw), uni, {}, {}, it)


# ------------------------------------------------------------------------------------------------ the with-flow model
from dataclasses import dataclass  # noqa: E402


@dataclass
class FlowParams:
    spec: op.PermutoSpec            # the flow lattice: in_dim 4, its own shifts (seed 1)
    grid: torch.Tensor              # f64, fp16-representable values
    w: torch.Tensor                 # flat f64 [64 x 2L | 64 x 64 | 6 x 64]
    b: torch.Tensor                 # flat f64 [64 | 64 | 6]

    def tensors(self):
        return [self.grid, self.w, self.b]


def make_flow_params(n_levels=6, log2_hashmap_size=10, coarsest_res=4.0, finest_res=32.0, seed=17, grid_bound=0.5) -> FlowParams:
    spec = op.make_permuto_spec(4, n_levels, 2, log2_hashmap_size, coarsest_res, finest_res, True, seed=1)
    g = torch.Generator().manual_seed(seed)
    grid = ((torch.rand(spec.n_params, generator=g) * 2 - 1) * grid_bound).half().double()
    w, b = make_flow_decoder(n_levels, seed + 1)
    return FlowParams(spec, grid, w.double(), b.double())


def _lattice(spec, grid, aabb, x, w, n_active=None):
    c, h = (aabb[0] + aabb[1]) * 0.5, (aabb[1] - aabb[0]) * 0.5
    x4 = torch.cat([(x.double() - c) / h, w.double().reshape(-1, 1)], dim=-1)
    return active_features(x4, grid, spec, n_active)


def flow_at(fp: FlowParams, aabb, x, w) -> torch.Tensor:
    """flow6 [S,6] at positions x (object coordinates) and time codes w: the flow lattice sees the AABB-normalised position"""
    return flow_decoder(_lattice(fp.spec, fp.grid, aabb, x, w), fp.w, fp.b)


def query_points(p, fp: FlowParams, x, ts, view_dirs=None, h_appear=None, step=0.1):
    """The with-flow query of DESIGN.md sec. 7 at points x [S,3] with times ts [S] -> sigma, opacity_alpha (, rgb) and the four
    flow tensors.  ``p``: dynamic_nerf_ref.DynParams."""
    w = dref.time_coord(p.ts_keyframes, p.codes, ts)
    T = int(p.codes.shape[0])
    lo, hi = float(p.codes[0]), float(p.codes[-1]) if T > 1 else float(p.codes[0])
    if T == 1:
        lo, hi = -1.0, 1.0                       # (the range of the config: with one keyframe delta is 0 and nothing clamps)
    delta, wp, wm = time_neighbours(w, T, lo, hi)
    x = x.double()
    f6 = flow_at(fp, p.aabb, x, w)
    xp, xm = x + f6[:, :3], x + f6[:, 3:]
    pp, pm = flow_at(fp, p.aabb, xp, wp), flow_at(fp, p.aabb, xm, wm)
    w1, b1, w2, b2 = p.den_w[0], p.den_b[0], p.den_w[1], p.den_b[1]

    def hidden(xx, ww):
        return torch.relu(_lattice(p.spec, p.grid, p.aabb, xx, ww, p.n_active) @ w1.t() + b1)
    a = 0.5 * hidden(x, w) + 0.25 * hidden(xp, wp) + 0.25 * hidden(xm, wm)
    out = a @ w2.t() + b2
    raw = out[:, 0]
    sigma = dref.trunc_softplus(raw)
    ret = dict(sigma=sigma, raw=raw, opacity_alpha=1.0 - torch.exp(-sigma * step), w=w, flow_fwd=f6[:, :3], flow_fwd_pred_bwd=pp[:, 3:],
               flow_bwd=f6[:, 3:], flow_bwd_pred_fwd=pm[:, :3])
    if view_dirs is not None:
        ret["rgb"] = dref.radiance(p, out[:, 1:], view_dirs, h_appear)
    return ret
